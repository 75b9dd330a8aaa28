"""Signed normal sources on the GPU (include/itw_dispatch.h, "signed normal sources"; include/itw_bc45.h): itwQuantizeNormalMapChain against
the numpy model (tests/_normal_snorm.py), and itwCompressNormalMapBC5S against CompressBlocksBC5S of the model's int8 image and, on the
small sizes, against the reference's D3DXEncodeBC5S (tests/_dxtex_snorm.py).  Every comparison is ==.  On the parent commit neither symbol
exists: every case here fails there."""
import ctypes as C
import os

import numpy as np
import pytest

import _dxtex_snorm as D
import _guarded as G
import _normal_snorm as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
f32 = np.float32
KINDS = S.KINDS
content = S.content
_torch_of = S.torch_of
_cache = {}


def _hash8(n, seed):
    i = np.arange(n, dtype=np.uint32)
    return ((i + np.uint32(seed)) * np.uint32(2654435761) >> np.uint32(13)).astype(np.uint32)


# ---- the sweep sources ------------------------------------------------------------------------------------------------------------------

def half_sweep():
    """256 x 256 RGBA16F bit patterns: R every half pattern once, G the same reversed, B and A hashed (NaN and +-Inf are in it)"""
    if "half" not in _cache:
        r = np.arange(65536, dtype=np.uint16)
        h = _hash8(65536, 1)
        _cache["half"] = np.stack([r, r[::-1], (h & 0xffff).astype(np.uint16), (h >> 16).astype(np.uint16)], axis=1).reshape(256, 256, 4).copy()
    return _cache["half"]


def float_sweep():
    """64 x 32 RGBA32F: fp32((k + 0.5) / 127), k = -127 .. 126, with three neighbours on either side, and the special values, in each of the
    four components (each component walks the list from another start, so the normalise sees mixed vectors)"""
    if "float" not in _cache:
        k = np.arange(-127, 127, dtype=np.float64)
        mid = ((k + 0.5) / 127.0).astype(f32)
        pts = [mid]
        lo = hi = mid
        for _ in range(3):
            lo = np.nextafter(lo, f32(-2.0))
            hi = np.nextafter(hi, f32(2.0))
            pts += [lo, hi]
        one = f32(1.0)
        special = np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(one, f32(2)), np.nextafter(-one, f32(-2)), 2.0, -2.0, 1e-45, np.inf, -np.inf, np.nan], dtype=f32)
        vals = np.concatenate([np.stack(pts, axis=1).reshape(-1), special])
        assert vals.size <= 2048 and np.isnan(vals).sum() == 1
        vals = np.concatenate([vals, np.zeros(2048 - vals.size, f32)])
        _cache["float"] = np.stack([np.roll(vals, 601 * c) for c in range(4)], axis=1).reshape(32, 64, 4).copy()
    return _cache["float"]


def int8_sweep():
    """256 x 256 RGBA8_SNORM: every (x, y) pair, z from seven values by row band, alpha hashed"""
    if "int8" not in _cache:
        img = np.empty((256, 256, 4), np.int8)
        c = np.arange(256).astype(np.uint8).view(np.int8)
        img[..., 0] = c[None, :]
        img[..., 1] = c[:, None]
        z = np.array([-128, -127, -1, 0, 1, 64, 127], np.int8)
        img[..., 2] = z[(np.arange(256) * 7) // 256][:, None]
        img[..., 3] = (_hash8(65536, 3) >> 8).astype(np.uint8).view(np.int8).reshape(256, 256)
        _cache["int8"] = img
    return _cache["int8"]


SWEEPS = [("half", 0), ("half", 7), ("float", 0), ("float", 7), ("int8", 4), ("int8", 7)]


@pytest.mark.parametrize("kind,ops", SWEEPS, ids=[f"{k}-ops{o}" for k, o in SWEEPS])
def test_quantiser_sweep(itw, gpu, kind, ops):
    import torch
    src = {"half": half_sweep, "float": float_sweep, "int8": int8_sweep}[kind]()
    want = S.quantize(src, ops)
    assert want.min() >= -127
    t = _torch_of(src, gpu)
    got = itw.quantize_normal_map(t, ops=ops)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[0].tolist(), src[tuple(bad[0][:2])].tolist(), got[tuple(bad[0][:2])].tolist(), want[tuple(bad[0][:2])].tolist())
    assert np.array_equal(t.cpu().numpy().view(np.uint8), src.view(np.uint8)), "the source was written"
    # the same source through the fused encoder as one whole image
    stream = itw.compress_normal_map_snorm(t, ops=ops).cpu().numpy()
    ref = itw.compress("bc5_snorm", torch.from_numpy(want).to(gpu)).cpu().numpy()
    bad = np.nonzero((stream.reshape(-1, 16) != ref.reshape(-1, 16)).any(axis=1))[0]
    assert bad.size == 0, (bad.size, int(bad[0]))


def test_ties_are_in_the_float_sweep_and_decide_codes():
    """the sweep separates round-to-nearest-even from round-half-away: some of its points are exact k + 0.5 products and the two rules differ there"""
    v = float_sweep()[..., 0].reshape(-1)
    v = v[np.isfinite(v) & (np.abs(v) < 1)]
    p = (v * f32(127.0)).astype(np.float64)
    tie = (p - np.floor(p)) == 0.5
    away = np.sign(p) * np.floor(np.abs(p) + 0.5)
    assert tie.sum() > 100 and (np.rint(p)[tie] != away[tie]).any()


# ---- the encoder --------------------------------------------------------------------------------------------------------------------------------------------

def want_stream(itw, gpu, src, ops, dxtex_too):
    """CompressBlocksBC5S of the model's image; on small sizes also checked against D3DXEncodeBC5S"""
    import torch
    q = np.ascontiguousarray(S.quantize(src, ops))
    want = itw.compress("bc5_snorm", torch.from_numpy(q).to(gpu)).cpu().numpy()
    if dxtex_too:
        assert np.array_equal(want, D.encode(2, q))
    return want


def surface(itw, ptr, w, h, stride):
    return itw.RgbaSurface(ptr, w, h, stride)


def assert_blocks(got, want, what):
    bad = np.nonzero((got.reshape(-1, 16) != want.reshape(-1, 16)).any(axis=1))[0]
    assert bad.size == 0, (what, bad.size, int(bad[0]), got.reshape(-1, 16)[bad[0]].tobytes().hex(), want.reshape(-1, 16)[bad[0]].tobytes().hex())


SIZES = [(1, 1), (3, 5), (5, 3), (4, 4), (61, 75)]       # (width, height)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("ops", [0, 3, 4, 7])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_stream_host_and_device_with_guards(itw, gpu, kind, ops, size):
    import torch
    w, h = size
    src = content(kind, h, w, 100 * h + w)
    want = want_stream(itw, gpu, src, ops, True)
    # device pointers: dst between guards, the source frozen
    fs = G.frozen(_torch_of(src, gpu))
    out = G.guarded(want.size, device=gpu)
    itw.compress_normal_map_snorm(fs.view, ops=ops, out=out.view)
    torch.cuda.synchronize()
    out.check("device dst")
    fs.check("device src")
    assert_blocks(out.host(), want, (kind, ops, size, "device"))
    # host pointers
    hs = G.frozen(src.view(np.int16) if src.dtype == np.uint16 else src)
    hout = G.guarded(want.size)
    itw.compress_normal_map_snorm(hs.view, ops=ops, out=hout.view)
    hout.check("host dst")
    hs.check("host src")
    assert_blocks(hout.host(), want, (kind, ops, size, "host"))
    assert itw.last_error() is None


@pytest.mark.parametrize("ops", [0, 3, 4, 7])
@pytest.mark.parametrize("kind", KINDS)
def test_a_view_one_texel_into_the_rows_takes_the_plain_loads(itw, gpu, kind, ops):
    """64 x 64 starting one texel into the rows of a 96-texel canvas: int8 and half rows start 4 / 8 bytes off a 16-byte address"""
    import torch
    canvas = content(kind, 64, 96, 9)
    src = canvas[:, 1:65]
    want = want_stream(itw, gpu, np.ascontiguousarray(src), ops, True)
    t = _torch_of(canvas, gpu)
    view = t[:, 1:65]
    assert view.data_ptr() % 16 == (0 if kind == "float" else src.dtype.itemsize * 4)
    got = itw.compress_normal_map_snorm(view, ops=ops).cpu().numpy()
    assert_blocks(got, want, (kind, ops, "device view"))
    hv = (canvas.view(np.int16) if canvas.dtype == np.uint16 else canvas)[:, 1:65]
    assert_blocks(itw.compress_normal_map_snorm(hv, ops=ops), want, (kind, ops, "host view"))


@pytest.mark.parametrize("ops", [0, 3, 4, 7])
@pytest.mark.parametrize("kind", KINDS)
def test_a_bottom_up_view(itw, gpu, kind, ops):
    """16 x 8 read from its last row upwards (negative stride), host and device"""
    import torch
    img = content(kind, 8, 16, 5)
    flipped = np.ascontiguousarray(img[::-1])
    want = want_stream(itw, gpu, flipped, ops, True)
    tb = S.texel_bytes(img)
    row = 16 * tb
    out = np.zeros(want.size, np.uint8)
    itw.lib().itwCompressNormalMapBC5S(C.byref(surface(itw, img.ctypes.data + 7 * row, 16, 8, -row)), tb, out.ctypes.data, ops)
    assert_blocks(out, want, (kind, ops, "host"))
    t = _torch_of(img, gpu)
    dout = torch.zeros(want.size, dtype=torch.uint8, device=gpu)
    itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
    itw.lib().itwCompressNormalMapBC5S(C.byref(surface(itw, t.data_ptr() + 7 * row, 16, 8, -row)), tb, dout.data_ptr(), ops)
    torch.cuda.synchronize()
    assert_blocks(dout.cpu().numpy(), want, (kind, ops, "device"))
    assert itw.last_error() is None


def normals128(kind):
    """128 x 128 from the golden normal map, recentred to signed values"""
    n = np.load(os.path.join(ROOT, "tests", "golden", "samples2.npz"))["normals"][64:192, 64:192]
    v = (n.astype(f32) - f32(128.0)) * (f32(1.0) / f32(127.0))
    if kind == "int8":
        return np.ascontiguousarray((n.astype(np.int32) - 128).astype(np.int8))
    return np.ascontiguousarray(v.astype(np.float16).view(np.uint16) if kind == "half" else v)


@pytest.mark.parametrize("ops", [0, 3, 4, 7])
@pytest.mark.parametrize("kind", KINDS)
def test_a_normal_map_crop(itw, gpu, kind, ops):
    src = normals128(kind)
    want = want_stream(itw, gpu, src, ops, True)
    assert_blocks(itw.compress_normal_map_snorm(_torch_of(src, gpu), ops=ops).cpu().numpy(), want, (kind, ops))


def test_int8_with_no_ops_is_compress_blocks_bc5s(itw, gpu):
    import torch
    src = content("int8", 75, 61, 7575)
    t = torch.from_numpy(src).to(gpu)
    assert np.array_equal(itw.compress_normal_map_snorm(t, ops=0).cpu().numpy(), itw.compress("bc5_snorm", t).cpu().numpy())


@pytest.mark.parametrize("kind", KINDS)
def test_device_call_is_capturable_after_warmup(itw, gpu, kind):
    import torch
    itw.lib().itwWarmupBC45S()
    assert itw.last_error() is None
    src = content(kind, 64, 64, 11)
    want = want_stream(itw, gpu, src, 7, True)
    d = _torch_of(src, gpu)
    out = torch.zeros(want.size, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        itw.compress_normal_map_snorm(d, ops=7, out=out)
    torch.cuda.synchronize()
    for replays in (1, 3):
        out.zero_()
        for _ in range(replays):
            g.replay()
        torch.cuda.synchronize()
        assert_blocks(out.cpu().numpy(), want, (kind, replays))
    assert itw.last_error() is None


@pytest.mark.parametrize("kind", KINDS)
def test_a_surface_of_more_chunks_than_workgroups_takes_the_prefetch_loop(itw, gpu, kind):
    """2052 x 2056: 263 682 blocks = 2 061 chunks of 128 blocks over 2 048 persistent workgroups, so 13 workgroups take a second, prefetched
    chunk and the last chunk is partial.  Against CompressBlocksBC5S of the model's image."""
    w, h = 2052, 2056
    assert (w // 4) * (h // 4) == 263682 and -(-263682 // 128) == 2061
    rng = np.random.default_rng(2052)
    v = rng.normal(0, 0.5, (h, w, 4)).astype(f32)
    v[rng.integers(0, 16, (h, w)) == 0, :3] = 0
    src = {"int8": lambda: np.clip(np.rint(v * 127), -128, 127).astype(np.int8), "half": lambda: v.astype(np.float16).view(np.uint16), "float": lambda: v}[kind]()
    want = want_stream(itw, gpu, src, 7, False)
    t = _torch_of(src, gpu)
    assert_blocks(itw.compress_normal_map_snorm(t, ops=7).cpu().numpy(), want, kind)
    assert np.array_equal(t.cpu().numpy().view(src.dtype), src)


# ---- the quantise call over chains -----------------------------------------------------------------------------------------------------------

CHAIN = [(37, 21), (18, 10), (9, 5), (4, 2), (2, 1), (1, 1)]        # (width, height)


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("kind", KINDS)
def test_quantise_a_chain_of_strided_views_writes_only_its_texels(itw, gpu, kind, where):
    import torch
    srcs = [content(kind, h, w, 31 * w + h) for w, h in CHAIN]
    wants = [S.quantize(s, 7) for s in srcs]
    dev = gpu if where == "device" else None
    fsrc = [G.frozen(s.view(np.int16) if s.dtype == np.uint16 else s, row_pad=S.texel_bytes(s) * 3, device=dev) for s in srcs]
    outs = [G.guarded(h * (4 * w + 12), device=dev, rows=(h, 4 * w, 4 * w + 12)) for w, h in CHAIN]
    src_arr = (itw.RgbaSurface * len(CHAIN))(*[surface(itw, f.ptr, w, h, f.stride) for f, (w, h) in zip(fsrc, CHAIN)])
    dst_arr = (itw.RgbaSurface * len(CHAIN))(*[surface(itw, o.ptr, w, h, 4 * w + 12) for o, (w, h) in zip(outs, CHAIN)])
    if dev is not None:
        itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
    assert itw.lib().itwQuantizeNormalMapChain(C.cast(src_arr, C.c_void_p), S.texel_bytes(srcs[0]), C.cast(dst_arr, C.c_void_p), len(CHAIN), 7) == 0
    if dev is not None:
        torch.cuda.synchronize()
    for f, o, want, size in zip(fsrc, outs, wants, CHAIN):
        o.check(f"target {size}")
        f.check(f"source {size}")
        assert np.array_equal(G.rows_of(o, np.int8).reshape(want.shape), want), size


@pytest.mark.parametrize("where", ["device", "host"])
def test_quantise_int8_in_place(itw, gpu, where):
    import torch
    srcs = [content("int8", h, w, 77 * w + h) for w, h in CHAIN]
    wants = [S.quantize(s, 7) for s in srcs]
    work = [torch.from_numpy(s).to(gpu) if where == "device" else s.copy() for s in srcs]
    res = itw.quantize_normal_map(work, ops=7, out=work)
    if where == "device":
        torch.cuda.synchronize()
    for r, want in zip(res, wants):
        assert np.array_equal(r.cpu().numpy() if where == "device" else r, want)


def test_quantise_refuses_mixed_host_and_device_pointers(itw, gpu):
    """returns -1 with a message; the targets stay as they were.  The error mode is process-wide: put back after the call."""
    import torch
    src = content("float", 8, 8, 1)
    dst = torch.full((8, 8, 4), 0x5A, dtype=torch.int8, device=gpu)
    s = surface(itw, src.ctypes.data, 8, 8, 128)
    d = surface(itw, dst.data_ptr(), 8, 8, 32)
    itw.set_error_mode(itw.ON_ERROR_RETURN)
    try:
        assert itw.lib().itwQuantizeNormalMapChain(C.byref(s), 16, C.byref(d), 1, 7) == -1
        assert "host or all device" in (itw.last_error() or "")
    finally:
        itw.lib().itwClearError()
        itw.set_error_mode(itw.ON_ERROR_ABORT)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 0x5A).all()
