"""itwDecodeBlocks is a chain of one through the kernel behind itwDecodeImage / itwDecodeChain (csrc/decode_chain.hip).  What that move can
break and the older suites do not hold: the three entry points agreeing block for block, BC6H_SF16 (96) read as unsigned by
itwDecodeBlocks alone, an output that is only 4-byte aligned (the dword-store path under itwDecodeBlocks' own argument rules), and every
mix of host and device pointers.  Every comparison is ==; the expected texels are the oracle's (tests/test_gpu_decode_chain.py::_want_image).
Not covered: a device failure inside itwDecodeBlocks in return mode (-1 and itwLastError) -- a failure is not to be provoked."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _block_sweep as sweep
from _guarded import guarded
from test_gpu_decode_chain import FORMATS, _random_blocks, _want_image

pytestmark = pytest.mark.gpu

PARTIAL = ("bc4", "bc5", "bc4_snorm", "bc5_snorm")
_cache = {}


def _blocks64(itw, fmt):
    """64 blocks: bc1 / bc3 random, the others spread evenly over the format's sweep stream (tests/_block_sweep.py); for bc7 / bc6h the
    last ones are the first block of every mode in ascending order and then a reserved block."""
    if fmt in ("bc1", "bc3"):
        return _random_blocks(itw, fmt, 64, 4242)
    blocks, w, h = getattr(sweep, fmt.split("_")[0])()
    bpb = itw.BYTES_PER_BLOCK[fmt]
    must = []
    if fmt in ("bc7", "bc6h"):
        built = sweep.bc7_modes() if fmt == "bc7" else sweep.bc6h_modes()
        must = [int(np.flatnonzero(built == m)[0]) for m in list(range(8 if fmt == "bc7" else 14)) + [-1]]
    pick = np.concatenate([np.linspace(0, blocks.size // bpb - 1, 64 - len(must)).astype(np.int64), np.array(must, dtype=np.int64)])
    return np.ascontiguousarray(blocks.reshape(-1, bpb)[pick]).reshape(-1)


def _tiles(img):
    """(h, w, 4) -> (blocks in raster order, 4, 4, 4)"""
    h, w, c = img.shape
    return img.reshape(h // 4, 4, w // 4, 4, c).swapaxes(1, 2).reshape(-1, 4, 4, c)


def _three_routes_case(itw, oracle, fmt):
    """[(16 blocks, their 32 x 8 texels, their modes)] * 4, computed once"""
    if fmt not in _cache:
        bpb = itw.BYTES_PER_BLOCK[fmt]
        all64 = _blocks64(itw, fmt)
        groups = []
        for g in range(4):
            blocks = np.ascontiguousarray(all64[g * 16 * bpb:(g + 1) * 16 * bpb])
            texels, modes = _want_image(oracle, fmt, blocks, 8, 32)
            groups.append((blocks, texels, modes))
        _cache[fmt] = groups
    return _cache[fmt]


@pytest.mark.parametrize("fmt", FORMATS)
def test_three_routes_one_answer(itw, gpu, oracle, fmt):
    """32 x 8 texels, 16 blocks: itwDecodeBlocks, itwDecodeImage and itwDecodeChain (the stream as two 16 x 8 images of 8 blocks each)
    give the oracle's texels, block for block, and its modes."""
    import torch
    for blocks, want, want_modes in _three_routes_case(itw, oracle, fmt):
        d = torch.from_numpy(blocks).to(gpu)
        a, am = itw.decode(fmt, d, 32, 8, want_modes=True)
        b, bm = itw.decode_image(fmt, d, (8, 32), want_modes=True)
        halves, cm = itw.decode_chain(fmt, d, [(8, 16), (8, 16)], want_modes=True)
        torch.cuda.synchronize()
        a, b = a.cpu().numpy().view(want.dtype), b.cpu().numpy().view(want.dtype)
        assert np.array_equal(a, want), (fmt, "itwDecodeBlocks", np.argwhere(a != want)[:4].tolist())
        assert np.array_equal(b, want), (fmt, "itwDecodeImage", np.argwhere(b != want)[:4].tolist())
        chain_tiles = np.concatenate([_tiles(t.cpu().numpy().view(want.dtype)) for t in halves])
        assert np.array_equal(chain_tiles, _tiles(want)), (fmt, "itwDecodeChain")
        for m, name in ((am, "itwDecodeBlocks"), (bm, "itwDecodeImage"), (cm, "itwDecodeChain")):
            assert np.array_equal(m.cpu().numpy(), want_modes), (fmt, name, "modes")
        h, hm = itw.decode(fmt, blocks, 32, 8, want_modes=True)                         # and itwDecodeBlocks through host pointers
        assert np.array_equal(h, want) and np.array_equal(hm, want_modes), (fmt, "itwDecodeBlocks, host")
    assert itw.last_error() is None


def test_bc6h_sf16_reads_as_unsigned_through_decode_blocks_only(itw, gpu, oracle):
    """96 through itwDecodeBlocks gives the bytes 95 gives (the signed decode is not built); itwDecodeImage still refuses 96."""
    import torch
    L = itw.lib()
    blocks = np.ascontiguousarray(_blocks64(itw, "bc6h")[-4 * 16:])                     # 8 x 8 texels; the last block is a reserved one
    want, want_modes = _want_image(oracle, "bc6h", blocks, 8, 8)
    d = torch.from_numpy(blocks).to(gpu)
    L.itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
    got = {}
    for f in (95, 96):
        out = torch.full((8, 8, 4), 0x5A5A, dtype=torch.int16, device=gpu)
        modes = torch.full((4,), 99, dtype=torch.int32, device=gpu)
        assert L.itwDecodeBlocks(f, d.data_ptr(), 8, 8, out.data_ptr(), 64, modes.data_ptr()) == 0
        torch.cuda.synchronize()
        got[f] = (out.cpu().numpy().view(np.uint16), modes.cpu().numpy())
    assert np.array_equal(got[95][0], want) and np.array_equal(got[95][1], want_modes)
    assert got[96][0].tobytes() == got[95][0].tobytes() and np.array_equal(got[96][1], got[95][1])
    out = torch.full((8, 8, 4), 0x5A5A, dtype=torch.int16, device=gpu)
    surf = itw.RgbaSurface(out.data_ptr(), 8, 8, 64)
    assert L.itwDecodeImage(96, d.data_ptr(), C.byref(surf), None, None) == -1
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A).all())


UNALIGNED = [(f, 8, 8) for f in FORMATS] + [(f, 5, 7) for f in PARTIAL]


@pytest.mark.parametrize("fmt,w,h", UNALIGNED, ids=[f"{f}-{w}x{h}" for f, w, h in UNALIGNED])
def test_decode_blocks_into_an_output_off_its_alignment(itw, gpu, oracle, fmt, w, h):
    """Everything on the device; `out` 4 bytes past a 16-byte boundary (8 for bc6h) and rows 4 (8) bytes apart from tight, so no row is
    16-byte aligned twice in a row: the kernel's dword stores.  The texels are the oracle's and every byte around and between the rows
    still holds the fill pattern, on two consecutive calls into a re-patterned buffer."""
    import torch
    px = 8 if fmt == "bc6h" else 4
    nb = ((w + 3) // 4) * ((h + 3) // 4)
    blocks = np.ascontiguousarray(_blocks64(itw, fmt)[-nb * itw.BYTES_PER_BLOCK[fmt]:])
    want, want_modes = _want_image(oracle, fmt, blocks, h, w)
    row_bytes, stride = w * px, w * px + px
    out = guarded(h * stride, device=gpu, offset=px, rows=(h, row_bytes, stride))
    modes = guarded(nb * 4, device=gpu)
    assert out.ptr % 16 == px and stride % 4 == 0 and stride % 16
    d = torch.from_numpy(blocks).to(gpu)
    itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
    for call in (1, 2):
        out.refill()
        modes.refill()
        assert itw.lib().itwDecodeBlocks(itw.DXGI_FORMAT[fmt], d.data_ptr(), w, h, out.ptr, stride, modes.ptr) == 0
        torch.cuda.synchronize()
        got = np.ascontiguousarray(out.host().reshape(h, stride)[:, :row_bytes]).view(want.dtype).reshape(h, w, 4)
        assert np.array_equal(got, want), (fmt, call, np.argwhere(got != want)[:4].tolist())
        assert np.array_equal(modes.host().view(np.int32), want_modes), (fmt, call)
        out.check(f"decode blocks {fmt} {w}x{h} call {call}: texels")
        modes.check(f"decode blocks {fmt} {w}x{h} call {call}: modes")
    assert itw.last_error() is None


@pytest.mark.parametrize("fmt", ["bc1", "bc7"])
def test_decode_blocks_takes_any_mix_of_host_and_device_pointers(itw, gpu, oracle, fmt):
    """8 x 8: all 8 host / device combinations of (blocks, out, modes) give the oracle's texels and modes."""
    import torch
    L = itw.lib()
    blocks = np.ascontiguousarray(_blocks64(itw, fmt)[-4 * itw.BYTES_PER_BLOCK[fmt]:])
    want, want_modes = _want_image(oracle, fmt, blocks, 8, 8)
    L.itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
    d_blocks = torch.from_numpy(blocks).to(gpu)
    for dev_b, dev_o, dev_m in itertools.product((False, True), repeat=3):
        out = torch.full((8, 8, 4), 0x5A, dtype=torch.uint8, device=gpu) if dev_o else np.full((8, 8, 4), 0x5A, dtype=np.uint8)
        modes = torch.full((4,), 99, dtype=torch.int32, device=gpu) if dev_m else np.full(4, 99, dtype=np.int32)
        ptr = lambda t: t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data       # noqa: E731
        assert L.itwDecodeBlocks(itw.DXGI_FORMAT[fmt], ptr(d_blocks if dev_b else blocks), 8, 8, ptr(out), 32, ptr(modes)) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy() if dev_o else out
        got_modes = modes.cpu().numpy() if dev_m else modes
        assert np.array_equal(got, want) and np.array_equal(got_modes, want_modes), (fmt, dev_b, dev_o, dev_m)
    assert itw.last_error() is None
