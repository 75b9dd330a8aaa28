"""itwCompressNormalMapBC5 (include/itw_bc45.h; csrc/bc4_bc5.hip, the PREP instantiations of bc45_kernel): the stream is byte for byte
CompressBlocksBC5 of a copy prepared by the numpy checker (tests/_normal_prep.py), and the reference encoder's (D3DXEncodeBC5U of
oracle/_ref/libdxtex_bc_ref.so) on that copy; the source is not modified; nothing is written outside the stream.  On the parent commit the
symbol does not exist: every case here fails there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _dxtex_snorm as D
import _normal_prep as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "oracle", "_ref", "libdxtex_bc_ref.so")
pytestmark = pytest.mark.gpu
GUARD = 256


@pytest.fixture(scope="module")
def dxtex():
    if not os.path.exists(LIB):
        if not os.path.exists("/root/reference/3rdParty/DirectXTex/DirectXTex/BC6HBC7.cpp"):
            pytest.skip("oracle/_ref/libdxtex_bc_ref.so not prebuilt and /root/reference absent")
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True)
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle", "ref_build")], check=True)
    L = C.CDLL(LIB)
    L.dxtex_ref_encode_bc45.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.dxtex_ref_encode_bc45.restype = None
    return L


def _reference_bc5(L, img):
    """DirectX::Compress of an RGBA8 image to BC5_UNORM: the partial-block fill, texel = code * (1 / 255), D3DXEncodeBC5U per block"""
    t = D.block_texels(img)[..., :2].astype(np.float32) * np.float32(1.0 / 255.0)
    out = np.zeros((t.shape[0], 16), np.uint8)
    for i in range(t.shape[0]):
        rg = np.ascontiguousarray(t[i], dtype=np.float32)
        L.dxtex_ref_encode_bc45(2, rg.ctypes.data, out[i].ctypes.data)
    return out.reshape(-1)


def _content(h, w, seed):
    """random texels, a quarter of them exact zero vectors / axis vectors / extreme codes, so that the default normal and both ends of the code range occur"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    k = rng.integers(0, 16, (h, w))
    img[k == 0, :3] = 128
    img[k == 1, :3] = [128, 128, 0]
    img[k == 2, :3] = [0, 255, 128]
    img[k == 3, :3] = [255, 0, 255]
    return img


# (height, width, row padding in texels): whole blocks, partial blocks, more than one workgroup, a view with a stride above the row
SHAPES = [(4, 4, 0), (8, 8, 0), (7, 5, 0), (1, 1, 0), (6, 8, 0), (64, 64, 0), (132, 260, 7)]      # (6 x 8: partial blocks behind 16-byte rows)
_cache = {}


def _case(shape):
    if shape not in _cache:
        h, w, pad = shape
        canvas = _content(h, w + pad, 1000 * h + w)
        _cache[shape] = canvas
    return _cache[shape]


def _fused_device(itw, gpu, view, ops):
    """the fused call on a device view; returns (stream, guard ok, source unchanged)"""
    import torch
    h, w = view.shape[:2]
    nbytes = itw.block_count("bc5", w, h) * 16
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    itw.compress_normal_map(view, ops=ops, out=buf[GUARD:GUARD + nbytes])
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert (b[:GUARD] == 0xA5).all() and (b[GUARD + nbytes:] == 0xA5).all(), "guard band around dst"
    return b[GUARD:GUARD + nbytes]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
@pytest.mark.parametrize("ops", range(8))
def test_fused_stream_is_bc5_of_the_prepared_copy(itw, gpu, dxtex, shape, ops):
    import torch
    h, w, pad = shape
    canvas = _case(shape)
    src = canvas[:, :w]
    prepared = np.ascontiguousarray(N.prepare_rgba8(src, ops))
    want = itw.compress("bc5", torch.from_numpy(prepared).to(gpu)).cpu().numpy()
    assert np.array_equal(want, _reference_bc5(dxtex, prepared))                 # the existing encoder is the reference's on this content
    # device pointers
    tc = torch.from_numpy(canvas).to(gpu)
    got = _fused_device(itw, gpu, tc[:, :w], ops)
    bad = np.nonzero((got.reshape(-1, 16) != want.reshape(-1, 16)).any(axis=1))[0]
    assert bad.size == 0, (ops, bad.size, int(bad[0]), got.reshape(-1, 16)[bad[0]].tobytes().hex(), want.reshape(-1, 16)[bad[0]].tobytes().hex())
    assert np.array_equal(tc.cpu().numpy(), canvas), "the source was written"
    if ops == 0:
        assert np.array_equal(got, itw.compress("bc5", tc[:, :w]).cpu().numpy())
    # host pointers
    keep = canvas.copy()
    out = np.full(got.size + 2 * GUARD, 0xA5, np.uint8)
    itw.compress_normal_map(canvas[:, :w], ops=ops, out=out[GUARD:GUARD + got.size])
    assert np.array_equal(out[GUARD:GUARD + got.size], want)
    assert (out[:GUARD] == 0xA5).all() and (out[GUARD + got.size:] == 0xA5).all()
    assert np.array_equal(canvas, keep)


@pytest.mark.parametrize("ops", [4, 7, 2])
def test_a_surface_of_more_chunks_than_workgroups_takes_the_prefetch_path(itw, gpu, ops):
    """2052 x 2048: 262 656 blocks = 2 052 chunks of 128 blocks, more than the 2 048 workgroups of the grid, so some workgroups walk a second chunk
    whose texels were requested by the prefetch."""
    import torch
    img = _content(2048, 2052, 77)
    assert (2052 // 4) * (2048 // 4) > 2048 * 128
    t = torch.from_numpy(img).to(gpu)
    want = itw.compress("bc5", torch.from_numpy(N.prepare_rgba8(img, ops)).to(gpu)).cpu().numpy()
    got = _fused_device(itw, gpu, t, ops)
    bad = np.nonzero((got.reshape(-1, 16) != want.reshape(-1, 16)).any(axis=1))[0]
    assert bad.size == 0, (bad.size, int(bad[0]))
    assert np.array_equal(t.cpu().numpy(), img)


def test_every_triple_through_the_fused_normalise(itw, gpu):
    """The scale table behind the fused normalise over its whole domain: the 4096^2 surface of all 2^24 triples."""
    import torch
    img = N.all_triples()
    want = itw.compress("bc5", torch.from_numpy(N.prepare_rgba8(img, N.NORMALIZE)).to(gpu)).cpu().numpy()
    got = itw.compress_normal_map(torch.from_numpy(img).to(gpu), normalize=True).cpu().numpy()
    bad = np.nonzero((got.reshape(-1, 16) != want.reshape(-1, 16)).any(axis=1))[0]
    assert bad.size == 0, (bad.size, int(bad[0]))
