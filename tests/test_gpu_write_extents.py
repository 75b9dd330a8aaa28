"""WHERE every device entry point writes: each caller-visible output lies between guard bands (tests/_guarded.py), each source in a
frozen buffer.  Every case checks three things -- the payload equals the reference the content tests use (the CPU oracle, byte for byte;
the library's own per-image calls for the two large chains), guards and row padding still hold the fill pattern, the sources are
unchanged -- and does so on two consecutive calls into a re-patterned buffer, so that the second call cannot lean on the first one's
bytes.  Sizes are the smallest at which a tail exists.  The multi-GPU entry points need two GPUs and are not covered here."""
import ctypes as C

import numpy as np
import pytest

from _guarded import frozen, guarded, pattern, rows_of
from conftest import first_mismatch
from test_gpu_chain import _oracle_chain, _per_image
from test_gpu_decode import _oracle_texels
from test_gpu_measure import _expect, _random_blocks, _random_source, _same
from test_prepass_convert import _oracle8, _oracle16, _source

pytestmark = pytest.mark.gpu

BPB = {"bc1": 8, "bc3": 16, "bc4": 8, "bc5": 16, "bc6h": 16, "bc7": 16}
# w x h: 1 block; 18 blocks in two block rows; 255 = one short of a workgroup; 65 = one lane into a second wave; 257 = one lane into a
# second workgroup
TAILS = [(4, 4), (36, 8), (68, 60), (260, 4), (1028, 4)]
PARTIAL = [(1, 1), (5, 3), (61, 62)]                             # BC4 / BC5 keep partial blocks
ROW_PAD = 48                                                     # source rows 48 bytes apart from tight: still 16-byte aligned

_cache = {}


def _content(fmt, prof, w, h):
    """ldr_smooth / hdr_smooth; the BC7 alpha profiles get a translucent left half, so that their RGB block list is neither empty nor full."""
    key = ("img", fmt, (prof or "").startswith("alpha"), w, h)
    if key not in _cache:
        from itw_amd import surfaces
        if fmt == "bc6h":
            img = surfaces.hdr_smooth(h, w, seed=surfaces.SEED + 51)
        else:
            img = surfaces.ldr_smooth(h, w, seed=surfaces.SEED + 51).copy()
            if key[2]:
                img[..., 3] = 255
                img[:, :max(1, w // 2), 3] = np.random.default_rng(w * 7 + h).integers(90, 170, (h, max(1, w // 2)))
        img.setflags(write=False)
        _cache[key] = img
    return _cache[key]


def _want(oracle, fmt, prof, w, h):
    key = ("enc", fmt, prof, w, h)
    if key not in _cache:
        img = _content(fmt, prof, w, h)
        _cache[key] = oracle.encode_bc45(fmt, img) if fmt in ("bc4", "bc5") else oracle.encode_mt(fmt, img, prof)
        _cache[key].setflags(write=False)
    return _cache[key]


def _twice(outs, srcs, call, compare, what):
    """Two rounds of: re-pattern every output, call, compare the payloads, check every guard and every source."""
    import torch
    for rnd in (1, 2):
        for o in outs:
            o.refill()
        call()
        torch.cuda.synchronize()
        compare((what, f"call {rnd}"))
        for k, o in enumerate(outs):
            o.check(f"{what}, call {rnd}, output {k}")
        for k, s in enumerate(srcs):
            s.check(f"{what}, call {rnd}, source {k}")


def _blocks_equal(out, want, fmt, what):
    got = out.host()
    assert got.size == want.size, (what, got.size, want.size)
    m = first_mismatch(got, want, BPB[fmt])
    assert m is None, (what, m)


@pytest.fixture
def paths(itw):
    yield itw.set_bc7_path
    itw.set_bc7_path("auto")


# ---- A. CompressBlocks*, device -> device ------------------------------------------------------------------------------------------

def _encode_on_device(itw, gpu, oracle, fmt, prof, w, h, offset, what):
    want = _want(oracle, fmt, prof, w, h)
    src = frozen(_content(fmt, prof, w, h), row_pad=ROW_PAD, device=gpu)
    out = guarded(want.size, device=gpu, offset=offset)
    assert src.ptr % 16 == 0 and (src.stride % 16 == 0 or w % 4) and out.ptr % 16 == offset     # (rows of a partial width: 4-byte aligned)
    _twice([out], [src], lambda: itw.compress(fmt, src.view, prof, out=out.view), lambda at: _blocks_equal(out, want, fmt, at), what)


SIMPLE = [(f, None, w, h) for f in ("bc1", "bc3", "bc4", "bc5") for w, h in TAILS] + [(f, None, w, h) for f in ("bc4", "bc5") for w, h in PARTIAL]


@pytest.mark.parametrize("fmt,prof,w,h", SIMPLE, ids=[f"{f}-{w}x{h}" for f, p, w, h in SIMPLE])
def test_a_bc1_bc3_bc4_bc5_device(itw, gpu, oracle, fmt, prof, w, h):
    _encode_on_device(itw, gpu, oracle, fmt, prof, w, h, 0, f"{fmt} {w}x{h}")


@pytest.mark.parametrize("w,h", TAILS, ids=[f"{w}x{h}" for w, h in TAILS])
@pytest.mark.parametrize("path", ["deep", "wide"])
@pytest.mark.parametrize("prof", ["veryfast", "basic", "slow", "alpha_basic", "alpha_slow"])
def test_a_bc7_device(itw, gpu, oracle, paths, prof, path, w, h):
    paths(path)
    _encode_on_device(itw, gpu, oracle, "bc7", prof, w, h, 0, f"bc7 {prof} {path} {w}x{h}")


@pytest.mark.parametrize("w,h", TAILS, ids=[f"{w}x{h}" for w, h in TAILS])
@pytest.mark.parametrize("path", ["deep", "wide"])
@pytest.mark.parametrize("prof", ["fast", "slow"])
def test_a_bc6h_device(itw, gpu, oracle, paths, prof, path, w, h):
    paths(path)
    _encode_on_device(itw, gpu, oracle, "bc6h", prof, w, h, 0, f"bc6h {prof} {path} {w}x{h}")


# the formats whose launch code looks at the destination's alignment (BC1: 8 bytes, the others 16) -> the dword-store kernels, same bytes
UNALIGNED = [("bc1", None, 4, "auto"), ("bc3", None, 4, "auto"), ("bc3", None, 8, "auto")] + \
            [(f, p, o, path) for f, p, o in (("bc7", "veryfast", 4), ("bc7", "slow", 4), ("bc7", "alpha_basic", 4), ("bc6h", "fast", 8), ("bc6h", "slow", 8))
             for path in ("deep", "wide")]


@pytest.mark.parametrize("fmt,prof,offset,path", UNALIGNED, ids=[f"{f}-{p or '-'}+{o}-{path}" for f, p, o, path in UNALIGNED])
def test_a_destination_off_its_alignment(itw, gpu, oracle, paths, fmt, prof, offset, path):
    paths(path)
    _encode_on_device(itw, gpu, oracle, fmt, prof, 260, 4, offset, f"{fmt} {prof} {path} dst+{offset}")


# ---- B. the same entry points with host pointers -----------------------------------------------------------------------------------

HOSTED = [(f, p, w, h) for f, p in (("bc1", None), ("bc3", None), ("bc4", None), ("bc5", None), ("bc7", "basic"), ("bc6h", "slow"))
          for w, h in ((36, 8), (1028, 4))]


@pytest.mark.parametrize("fmt,prof,w,h", HOSTED, ids=[f"{f}-{w}x{h}" for f, p, w, h in HOSTED])
def test_b_host_pointers(itw, gpu, oracle, fmt, prof, w, h):
    want = _want(oracle, fmt, prof, w, h)
    src = frozen(_content(fmt, prof, w, h), row_pad=ROW_PAD)
    out = guarded(want.size)
    surf = itw.RgbaSurface(src.ptr, w, h, src.stride)
    _twice([out], [src], lambda: itw.abi._call(fmt, surf, out.ptr, prof), lambda at: _blocks_equal(out, want, fmt, at), f"host {fmt} {w}x{h}")


# ---- C. itwCompressImageSliced[Ex] ---------------------------------------------------------------------------------------------------

KINDS = [("host", "host"), ("device", "device"), ("host", "device"), ("device", "host")]
KIND_IDS = [f"{a}-to-{b}" for a, b in KINDS]
SLICED = [("bc1", None, 256, 192), ("bc7", "veryfast", 256, 192), ("bc6h", "fast", 256, 192), ("bc5", None, 256, 190)]
SLICE_PIXELS = 4096


def _slice_offsets(fmt, w, h):
    """Byte offset in the block stream at which each slice starts (include/itw_dispatch.h: rows [i*h/slices & ~3, (i+1)*h/slices & ~3))."""
    slices = w * h // SLICE_PIXELS
    bx = (w + 3) // 4 if fmt in ("bc4", "bc5") else w // 4
    return [((i * h // slices) & ~3) // 4 * bx * BPB[fmt] for i in range(slices)]


@pytest.fixture
def window_of_two(itw):
    itw.lib().itwSetSliceWindow(2)
    try:
        yield
    finally:
        itw.lib().itwSetSliceWindow(0)


@pytest.mark.parametrize("ex", [False, True], ids=["trampoline", "ex"])
@pytest.mark.parametrize("src_kind,dst_kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("fmt,prof,w,h", SLICED, ids=[f"{f}-{w}x{h}" for f, p, w, h in SLICED])
def test_c_sliced(itw, gpu, oracle, window_of_two, fmt, prof, w, h, src_kind, dst_kind, ex):
    want = _want(oracle, fmt, prof, w, h)
    slices = w * h // SLICE_PIXELS                                # 12 (11 for 256 x 190), in 6 windows
    assert slices in (11, 12) and itw.lib().itwSliceWindow(itw.DXGI_FORMAT[fmt], w, h, SLICE_PIXELS) == 2
    src = frozen(_content(fmt, prof, w, h), row_pad=ROW_PAD, device=gpu if src_kind == "device" else None)
    out = guarded(want.size, device=gpu if dst_kind == "device" else None)
    settings = None
    if ex and fmt in ("bc7", "bc6h"):
        settings = itw.bc7_profile(prof) if fmt == "bc7" else itw.bc6h_profile(prof)
    elif ex:
        settings = itw.Bc7Settings()                              # ignored for the other formats; selects the Ex entry point
    calls = []

    def call():
        del calls[:]
        ok, _ = itw.compress_image(fmt, src.view, prof, slice_pixels=SLICE_PIXELS, out=out.view, settings=settings,
                                   progress=lambda i, t, u: calls.append((i, t)) or True)
        assert ok

    def compare(at):
        assert calls == [(i, slices) for i in range(1, slices)], at
        _blocks_equal(out, want, fmt, at)

    _twice([out], [src], call, compare, f"sliced {fmt} {src_kind}->{dst_kind}")

    # ... and without a progress callback: nothing can stop the job, so the kernels of every window store straight into a device target
    def quiet():
        ok, _ = itw.compress_image(fmt, src.view, prof, slice_pixels=SLICE_PIXELS, out=out.view, settings=settings)
        assert ok

    _twice([out], [src], quiet, lambda at: _blocks_equal(out, want, fmt, at), f"sliced {fmt} {src_kind}->{dst_kind}, no progress")


@pytest.mark.parametrize("src_kind,dst_kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("fmt,prof,w,h", SLICED, ids=[f"{f}-{w}x{h}" for f, p, w, h in SLICED])
def test_c_sliced_early_out_leaves_the_rest_unwritten(itw, gpu, oracle, window_of_two, fmt, prof, w, h, src_kind, dst_kind):
    """progress returns false at i = 5: slices 0 .. 4 are in `target`, and so is the rest of slice 4's window (slice 5); the windows in
    flight at that moment are drained and not copied back, so everything behind slice 5 still holds the fill pattern."""
    want = _want(oracle, fmt, prof, w, h)
    starts = _slice_offsets(fmt, w, h)
    src = frozen(_content(fmt, prof, w, h), row_pad=ROW_PAD, device=gpu if src_kind == "device" else None)
    out = guarded(want.size, device=gpu if dst_kind == "device" else None)
    calls = []

    def call():
        del calls[:]
        ok, _ = itw.compress_image(fmt, src.view, prof, slice_pixels=SLICE_PIXELS, out=out.view,
                                   progress=lambda i, t, u: calls.append(i) or i != 5)
        assert ok is False

    def compare(at):
        assert calls == [1, 2, 3, 4, 5], at
        got = out.host()
        m = first_mismatch(got[:starts[5]], want[:starts[5]], BPB[fmt])
        assert m is None, (at, "slices < 5", m)
        rest = got[starts[6]:]                                    # slice 4's window is slices 4 and 5
        stale = np.flatnonzero(rest != pattern(rest.size, start=out.start + starts[6]))
        assert stale.size == 0, (at, f"{stale.size} bytes written behind the aborting window, payload offsets "
                                     f"{starts[6] + int(stale[0])} .. {starts[6] + int(stale[-1])} of {want.size}")

    _twice([out], [src], call, compare, f"sliced early out {fmt} {src_kind}->{dst_kind}")


# ---- D. itwCompressImageChain[Ex] ------------------------------------------------------------------------------------------------------

def _chain_images(itw, fmt, shape):
    key = ("chain", fmt == "bc6h", shape)
    if key not in _cache:
        from itw_amd import surfaces
        gen = surfaces.hdr_smooth if fmt == "bc6h" else surfaces.ldr_smooth
        if shape == "mips":                                       # a full chain of 37 x 21
            _cache[key] = itw.mip_chain(gen(21, 37, seed=surfaces.SEED + 61))
        else:                                                     # a cube map of 8 x 8 with mips, DDS order: face, then mip
            _cache[key] = [lv for f in range(6) for lv in itw.mip_chain(gen(8, 8, seed=surfaces.SEED + 70 + f))]
    return _cache[key]


CHAINED = [("bc1", None), ("bc4", None), ("bc7", "veryfast"), ("bc6h", "fast")]


@pytest.mark.parametrize("trampoline", [False, True], ids=["ex", "trampoline"])
@pytest.mark.parametrize("src_kind,dst_kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("shape", ["mips", "cube"])
@pytest.mark.parametrize("fmt,prof", CHAINED, ids=[f for f, p in CHAINED])
def test_d_chain(itw, gpu, oracle, fmt, prof, shape, src_kind, dst_kind, trampoline):
    levels = _chain_images(itw, fmt, shape)
    key = ("chain want", fmt, prof, shape)
    if key not in _cache:
        _cache[key] = _oracle_chain(itw, oracle, fmt, levels, prof)
    want = _cache[key]
    assert itw.chain_bytes(fmt, levels) == want.size
    srcs = [frozen(lv, row_pad=ROW_PAD, device=gpu if src_kind == "device" else None) for lv in levels]
    out = guarded(want.size, device=gpu if dst_kind == "device" else None)
    fn = itw.image_func(fmt, prof) if trampoline else None

    def call():
        ok, _ = itw.compress_chain(fmt, [s.view for s in srcs], prof, out=out.view, cmp_func=fn)
        assert ok

    _twice([out], srcs, call, lambda at: _blocks_equal(out, want, fmt, at), f"chain {fmt} {shape} {src_kind}->{dst_kind}")


@pytest.mark.parametrize("src_kind", ["host", "device"])
def test_d_chain_of_two_groups(itw, gpu, src_kind):
    """1462 x 1458: level 0 has 366 * 365 = 133 590 blocks -- a window's worth -- and is no multiple of 4, so it is gathered as a group
    of its own and the remaining levels form a second group.  Reference: the per-image loop of the library's own calls."""
    from itw_amd import surfaces
    if "two groups" not in _cache:
        levels = itw.mip_chain(surfaces.ldr_smooth(1458, 1462, seed=surfaces.SEED + 62))
        _cache["two groups"] = (levels, _per_image(itw, "bc7", levels, "veryfast"))
    levels, want = _cache["two groups"]
    assert ((1462 + 3) // 4) * ((1458 + 3) // 4) >= 131072
    srcs = [frozen(lv, row_pad=ROW_PAD, device=gpu if src_kind == "device" else None) for lv in levels]
    out = guarded(want.size, device=gpu)

    def call():
        ok, _ = itw.compress_chain("bc7", [s.view for s in srcs], "veryfast", out=out.view)
        assert ok

    _twice([out], srcs, call, lambda at: _blocks_equal(out, want, "bc7", at), f"two groups, {src_kind} images")


def test_d_chain_in_place_at_an_8_byte_aligned_destination(itw, gpu):
    """bc1, [4 x 4, 2048 x 2048]: the big aligned image is encoded in place, its blocks start at byte 8 of `target`."""
    from itw_amd import surfaces
    images = [surfaces.ldr_smooth(4, 4, seed=surfaces.SEED + 63), surfaces.ldr_smooth(2048, 2048, seed=surfaces.SEED + 64)]
    want = _per_image(itw, "bc1", images, None)
    srcs = [frozen(im, row_pad=ROW_PAD, device=gpu) for im in images]
    out = guarded(want.size, device=gpu)
    assert out.ptr % 16 == 0 and want.size == 8 + 262144 * 8

    def call():
        ok, _ = itw.compress_chain("bc1", [s.view for s in srcs], None, out=out.view)
        assert ok

    _twice([out], srcs, call, lambda at: _blocks_equal(out, want, "bc1", at), "in place at target + 8")


# ---- E. itwDecodeBlocks --------------------------------------------------------------------------------------------------------------

DECODED = [(f, w, h) for f in ("bc1", "bc3", "bc4", "bc5", "bc7", "bc6h") for w, h in ((4, 4), (260, 4), (1028, 8))] + \
          [(f, w, h) for f in ("bc4", "bc5") for w, h in PARTIAL]


def _decode_case(itw, oracle, fmt, w, h):
    key = ("dec", fmt, w, h)
    if key not in _cache:
        W, H = (w + 3) // 4 * 4, (h + 3) // 4 * 4
        nb = (W // 4) * (H // 4)
        blocks = _random_blocks(itw, fmt, nb, {"bc1": 1, "bc3": 3, "bc4": 4, "bc5": 5, "bc7": 7, "bc6h": 6}[fmt] + w)
        texels, modes = _oracle_texels(oracle, fmt, blocks, W, H)          # the padded size, cropped
        assert (modes >= -1).all()
        _cache[key] = (blocks, np.ascontiguousarray(texels[:h, :w]), modes)
    return _cache[key]


def _decode(itw, gpu, oracle, fmt, w, h, device):
    import torch
    blocks, want, want_modes = _decode_case(itw, oracle, fmt, w, h)
    row_bytes = w * (8 if fmt == "bc6h" else 4)
    stride = row_bytes + 64
    src = frozen(blocks, device=device)
    out = guarded(h * stride, device=device, rows=(h, row_bytes, stride))
    modes = guarded(want_modes.size * 4, device=device)
    itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)   # host pointers are staged on the thread's stream too

    def call():
        assert itw.lib().itwDecodeBlocks(itw.DXGI_FORMAT[fmt], src.ptr, w, h, out.ptr, stride, modes.ptr) == 0

    def compare(at):
        got = rows_of(out, want.dtype).reshape(h, w, 4)
        assert np.array_equal(got, want), (at, "texels", np.argwhere(got != want)[:4].tolist())
        assert np.array_equal(modes.host().view(np.int32), want_modes), (at, "modes")

    _twice([out, modes], [src], call, compare, f"decode {fmt} {w}x{h} {'device' if device is not None else 'host'}")


@pytest.mark.parametrize("fmt,w,h", DECODED, ids=[f"{f}-{w}x{h}" for f, w, h in DECODED])
def test_e_decode_into_a_strided_device_surface(itw, gpu, oracle, fmt, w, h):
    _decode(itw, gpu, oracle, fmt, w, h, gpu)


@pytest.mark.parametrize("fmt,w,h", [("bc3", 260, 4), ("bc5", 61, 62), ("bc6h", 260, 4)])
def test_e_decode_into_a_strided_host_surface(itw, gpu, oracle, fmt, w, h):
    _decode(itw, gpu, oracle, fmt, w, h, None)


# ---- F. itwMeasureBlocks / itwMeasureChain, all pointers on the device -------------------------------------------------------------

STATS_BYTES = 216


def _stats_buffer(itw, gpu, count=1):
    g = guarded(count * STATS_BYTES, device=gpu, offset=8)            # 8-byte aligned, as the header asks, and no more
    assert C.sizeof(itw.ErrorStats) == STATS_BYTES and g.ptr % 16 == 8
    return g


@pytest.mark.parametrize("w,h", [(5, 3), (260, 4), (1028, 4)], ids=["5x3", "260x4", "1028x4"])
@pytest.mark.parametrize("fmt", ["bc1", "bc5", "bc7", "bc6h"])
def test_f_measure_blocks(itw, gpu, oracle, fmt, w, h):
    import torch
    nb = ((w + 3) // 4) * ((h + 3) // 4)
    blocks = _random_blocks(itw, fmt, nb, 300 + w)
    texels = _random_source(fmt, h, w, 300 + w)
    want, want_map = _expect(itw, oracle, fmt, blocks, texels)
    d_blocks = frozen(blocks, device=gpu)
    d_src = frozen(texels, row_pad=ROW_PAD, device=gpu)
    stats = _stats_buffer(itw, gpu)
    bmap = guarded(nb * 8, device=gpu)

    def compare(at):
        _same(itw.ErrorStats.from_buffer_copy(stats.host().tobytes()), want, at)
        assert np.array_equal(bmap.host().view(np.uint64).astype(np.int64), want_map), (at, "block_sse")

    _twice([stats, bmap], [d_blocks, d_src],
           lambda: itw.measure_async(fmt, d_blocks.view, d_src.view, stats.view, bmap.view.view(torch.int64)), compare, f"measure {fmt} {w}x{h}")
    assert itw.last_error() is None


def test_f_measure_chain(itw, gpu, oracle):
    import torch
    levels = _chain_images(itw, "bc7", "mips")
    ok, stream = itw.compress_chain("bc7", levels, "veryfast")
    assert ok
    wants, off = [], 0
    for lv in levels:
        n = ((lv.shape[1] + 3) // 4) * ((lv.shape[0] + 3) // 4) * 16
        wants.append(_expect(itw, oracle, "bc7", stream[off:off + n], lv)[0])
        off += n
    assert off == stream.size
    d_blocks = frozen(stream, device=gpu)
    srcs = [frozen(lv, row_pad=ROW_PAD, device=gpu) for lv in levels]
    stats = _stats_buffer(itw, gpu, len(levels))
    arr = itw.abi._surfaces([s.view for s in srcs])
    itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)

    def call():
        assert itw.lib().itwMeasureChain(C.cast(arr, C.c_void_p), len(levels), d_blocks.ptr, itw.DXGI_FORMAT["bc7"], stats.ptr, STATS_BYTES) == 0

    def compare(at):
        raw = stats.host().tobytes()
        for i, want in enumerate(wants):
            _same(itw.ErrorStats.from_buffer_copy(raw[i * STATS_BYTES:(i + 1) * STATS_BYTES]), want, (at, i))

    _twice([stats], [d_blocks] + srcs, call, compare, "measure chain")


# ---- G. the pre-pass kernels -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pixel_size", [4, 8])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 7), (127, 9), (8, 4)], ids=["1x1", "5x7", "127x9", "8x4"])
def test_g_pad_to_multiple_of_4_on_the_device(itw, gpu, w, h, pixel_size):
    import torch
    rng = np.random.default_rng(w * 100 + h + pixel_size)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8) if pixel_size == 4 else rng.integers(0, 65536, (h, w, 4), dtype=np.uint16)
    W, H = (w + 3) & ~3, (h + 3) & ~3
    want = np.pad(img, ((0, H - h), (0, W - w), (0, 0)), mode="edge")
    src = frozen(img, row_pad=12 if pixel_size == 4 else 24, device=gpu)
    out = guarded(W * H * pixel_size, device=gpu)
    surf = itw.RgbaSurface(src.ptr, w, h, src.stride)
    itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)

    def compare(at):
        got = out.host().view(img.dtype).reshape(H, W, 4)
        assert np.array_equal(got, want), (at, np.argwhere(got != want)[:4].tolist())

    _twice([out], [src], lambda: itw.lib().itwPadToMultipleOf4Device(C.byref(surf), pixel_size, out.ptr), compare, f"pad {w}x{h} px{pixel_size}")
    assert itw.last_error() is None


@pytest.mark.parametrize("planes,alpha", [(1, 0), (3, 0), (4, 1)], ids=["1-plane", "3-planes", "4-planes"])
@pytest.mark.parametrize("depth", [8, 16, 32])
@pytest.mark.parametrize("w,h", [(1, 1), (257, 1), (203, 3)], ids=["1x1", "257x1", "203x3"])
def test_g_convert_on_the_device(itw, gpu, oracle, w, h, depth, planes, alpha):
    import torch
    L = itw.lib()
    host = _source(np.random.default_rng(depth + planes + w), depth, planes, max(w, 6), h)[:, :w]      # (_source plants six special values)
    host = np.ascontiguousarray(host)
    src = frozen(host, device=gpu)
    out8 = guarded(w * h * 4, device=gpu)
    out16 = guarded(w * h * 8, device=gpu)
    L.itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
    for gamma in ((0, 1) if depth == 32 else (0,)):
        want = _oracle8(oracle, host, depth, planes, alpha, gamma, w, h)

        def compare8(at):
            got = out8.host().reshape(h, w, 4)
            assert np.array_equal(got, want), (at, np.argwhere(got != want)[:4].tolist())

        _twice([out8], [src], lambda: L.itwConvertToRGBA8Device(src.ptr, depth, planes, alpha, gamma, w, h, out8.ptr) == 0 or pytest.fail("-1"),
               compare8, f"convert8 {w}x{h} depth {depth} planes {planes} gamma {gamma}")
    want16 = _oracle16(oracle, host, depth, planes, alpha, w, h)

    def compare16(at):
        got = out16.host().view(np.uint16).reshape(h, w, 4)
        assert np.array_equal(got, want16), (at, np.argwhere(got != want16)[:4].tolist())

    _twice([out16], [src], lambda: L.itwConvertToRGBA16FDevice(src.ptr, depth, planes, alpha, w, h, out16.ptr) == 0 or pytest.fail("-1"),
           compare16, f"convert16 {w}x{h} depth {depth} planes {planes}")
