"""itwDecodeBlocks and itwMeasureBlocks over the sweeps of tests/_block_sweep.py: every BC7 mode with every partition / rotation / index
selector, every BC6H (mode, partition) pair, the reserved blocks of both, every BC4 / BC5 endpoint pair under both readings, the BC1 / BC3
corner colours in both orders -- each with all-zero, all-one, alternating and random payloads.  The device decoders of
csrc/decode_core.hpp against the from-spec decoders of oracle/ and, where oracle/_ref/libdxtex_bc_ref.so travelled along, against
DirectXTex's own (tests/test_block_sweep.py shows the two agree on these streams).  Every comparison is `==`."""
import hashlib
import os

import numpy as np
import pytest

import _block_sweep as sweep
import _dxtex_snorm as snorm
from test_block_sweep import LIB, _half_to_float, _tiles, ref_decode
from test_gpu_bc45_snorm import _expect_stats
from test_gpu_measure import _expect, _random_source, _same, _to_gpu

pytestmark = pytest.mark.gpu

UNSIGNED = ["bc1", "bc3", "bc4", "bc5", "bc7", "bc6h"]
SIGNED = ["bc4_snorm", "bc5_snorm"]
NCH = {"bc4_snorm": 1, "bc5_snorm": 2}
_streams, _decoded = {}, {}


def _stream(fmt):
    """(blocks, width, height, modes the blocks were built as), generated once per format."""
    if fmt not in _streams:
        blocks, w, h = getattr(sweep, fmt.split("_")[0])(True) if fmt in SIGNED else getattr(sweep, fmt)()
        built = {"bc7": sweep.bc7_modes, "bc6h": sweep.bc6h_modes}.get(fmt, lambda: np.zeros((w // 4) * (h // 4), dtype=np.int32))()
        _streams[fmt] = (blocks, w, h, built)
    return _streams[fmt]


class _DecodesOnce:
    """The oracle fixture with decode() remembered per stream: the per-block CPU loop runs once for the tests that share a sweep."""

    def __init__(self, oracle):
        self._oracle = oracle

    def decode(self, fmt, blocks, w, h):
        key = (fmt, w, h, hashlib.sha1(np.ascontiguousarray(blocks).tobytes()).hexdigest())
        if key not in _decoded:
            dec, modes = self._oracle.decode(fmt, blocks, w, h)
            dec.setflags(write=False)
            modes.setflags(write=False)
            _decoded[key] = (dec, modes)
        return _decoded[key]


def _want_texels(oracle, fmt):
    blocks, w, h, _ = _stream(fmt)
    dec, modes = _DecodesOnce(oracle).decode(fmt, blocks, w, h)
    if fmt == "bc6h":                                            # the alpha fill, as in test_gpu_decode.py
        full = np.empty((h, w, 4), dtype=np.uint16)
        full[..., :3] = dec
        full[..., 3] = 0x3C00
        dec = full
    return dec, modes


def _decode_on_device(itw, gpu, fmt):
    import torch
    blocks, w, h, _ = _stream(fmt)
    got, modes = itw.decode(fmt, torch.from_numpy(blocks).to(gpu), w, h, want_modes=True)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    return (got.view(np.uint16) if fmt == "bc6h" else got), modes.cpu().numpy()


# ---- decode -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", UNSIGNED)
def test_sweep_decodes_like_the_oracle(itw, gpu, oracle, fmt):
    blocks, w, h, built = _stream(fmt)
    want, want_modes = _want_texels(oracle, fmt)
    assert np.array_equal(want_modes, built)                     # the oracle reads the modes the generator wrote; none malformed
    got, modes = _decode_on_device(itw, gpu, fmt)
    assert np.array_equal(modes, built)
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, (len(bad), [(int(y) // 4 * (w // 4) + int(x) // 4) for y, x in bad[:4]])
    if fmt == "bc7":                                             # host pointers: staged in, staged out
        host, host_modes = itw.decode(fmt, blocks, w, h, want_modes=True)
        assert np.array_equal(host, want) and np.array_equal(host_modes, built)


@pytest.mark.parametrize("fmt", SIGNED)
def test_sweep_decodes_by_the_signed_integer_rule(itw, gpu, fmt):
    blocks, w, h, built = _stream(fmt)
    got, modes = _decode_on_device(itw, gpu, fmt)
    assert got.dtype == np.int8
    assert np.array_equal(got, snorm.decode_int8(NCH[fmt], blocks, w, h))
    assert np.array_equal(modes, built)


@pytest.mark.parametrize("fmt,kind,nch", [("bc7", 7, 4), ("bc6h", 6, 3), ("bc4", 4, 1), ("bc5", 5, 2), ("bc4_snorm", None, 1), ("bc5_snorm", None, 2)])
def test_sweep_decodes_like_directxtex(itw, gpu, fmt, kind, nch):
    """The device decoders against D3DXDecodeBC7 / BC6HU / BC4U / BC5U / BC4S / BC5S directly, no oracle in between."""
    import ctypes as C
    if not os.path.exists(LIB):
        pytest.skip("oracle/_ref/libdxtex_bc_ref.so did not travel along")
    blocks, w, h, _ = _stream(fmt)
    got, _ = _decode_on_device(itw, gpu, fmt)
    mine = _tiles(got, w, h)[..., :nch]
    if fmt in SIGNED:
        ref = snorm.decode(nch, blocks)[..., :nch]
        assert np.array_equal(np.rint(127.0 * ref.astype(np.float64)).astype(np.int32), mine.astype(np.int32))
        return
    L = C.CDLL(LIB)
    L.dxtex_ref_decode.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.dxtex_ref_decode.restype = C.c_int
    ref, rc = ref_decode(L, kind, blocks, 16 if fmt != "bc4" else 8)
    assert not any(rc)
    if fmt == "bc6h":
        assert int(mine.max()) <= 0x7BFF
        assert np.array_equal(ref[..., :3], _half_to_float(mine))
    else:
        assert np.array_equal(np.rint(255.0 * ref[..., :nch].astype(np.float64)).astype(np.int32), mine.astype(np.int32))


# ---- measure ----------------------------------------------------------------------------------------------------------------------

def _source(fmt, h, w, kind):
    if kind == "zero":
        return np.zeros((h, w, 4), dtype=np.int8 if fmt in SIGNED else np.uint16 if fmt == "bc6h" else np.uint8)
    src = _random_source(fmt.split("_")[0], h, w, 77)
    return src.view(np.int8) if fmt in SIGNED else src           # every int8 code, -128 included


def _hist(built):
    return [int(v) for v in np.bincount(built[built >= 0], minlength=16)], int((built < 0).sum())


def _measure(itw, gpu, fmt, blocks, src):
    import torch
    st, bmap = itw.measure(fmt, _to_gpu(gpu, blocks), _to_gpu(gpu, src), want_block_map=True)
    torch.cuda.synchronize()
    return st, bmap.cpu().numpy()


@pytest.mark.parametrize("kind", ["zero", "random"])
@pytest.mark.parametrize("fmt", UNSIGNED)
def test_sweep_measures_like_numpy_on_the_oracles_decode(itw, gpu, oracle, fmt, kind):
    blocks, w, h, built = _stream(fmt)
    src = _source(fmt, h, w, kind)
    want, want_map = _expect(itw, _DecodesOnce(oracle), fmt, blocks, src)
    want["mode_hist"], want["reserved_blocks"] = _hist(built)   # from the generator's list, not from a decode
    assert sum(want["mode_hist"]) + want["reserved_blocks"] == want["blocks"] == built.size
    st, bmap = _measure(itw, gpu, fmt, blocks, src)
    _same(st, want, (fmt, kind))
    assert np.array_equal(bmap, want_map)


@pytest.mark.parametrize("kind", ["zero", "random"])
@pytest.mark.parametrize("fmt", SIGNED)
def test_signed_sweep_measures_like_numpy_on_the_integer_rule(itw, gpu, fmt, kind):
    blocks, w, h, built = _stream(fmt)
    src = _source(fmt, h, w, kind)
    want, want_map = _expect_stats(NCH[fmt], blocks, src)
    want.update(dxgi_format=itw.DXGI_FORMAT[fmt], width=w, height=h, reserved_blocks=0, mode_hist=[built.size] + [0] * 15)
    st, bmap = _measure(itw, gpu, fmt, blocks, src)
    _same(st, want, (fmt, kind))
    assert np.array_equal(bmap, want_map)


def test_bc7_sweep_measures_against_a_cropped_source(itw, gpu, oracle):
    """253 x 143: the last block column and row count one texel column / three texel rows; modes are counted for whole blocks."""
    blocks, w, h, built = _stream("bc7")
    src = _random_source("bc7", 143, 253, 78)
    want, want_map = _expect(itw, _DecodesOnce(oracle), "bc7", blocks, src)
    want["mode_hist"], want["reserved_blocks"] = _hist(built)
    assert want["blocks"] == built.size
    st, bmap = _measure(itw, gpu, "bc7", blocks, src)
    _same(st, want, "cropped")
    assert np.array_equal(bmap, want_map)
