"""ITW_MIP_SRGB on the device (include/itw_dispatch.h, "Mip chains"; csrc/mipgen.hpp, csrc/mipgen.hip): the kernels' encode against the
counting definition, both filters on both routes against the numpy model of tests/_srgb_mips.py, and the one-call save.  Every comparison
is == on bytes.  Every test that passes the flag fails on a build that refuses it."""
import ctypes as C
import functools

import numpy as np
import pytest

import _guarded as G
import _mipgen as M
import _srgb_mips as S

pytestmark = pytest.mark.gpu
F = np.float32


def _dev(gpu, a):
    import torch
    return torch.from_numpy(a).to(gpu)


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def test_the_device_encode_is_the_counting_definition(itw, gpu):
    """Every T[k] and the 3 floats either side, +-0, the smallest denormal, 1.0 and the next float up, 1.5, and 2^20 seeded floats in [0, 1]."""
    import torch
    values = np.concatenate([S.threshold_neighbourhood(3), np.random.default_rng(20).random(1 << 20, dtype=F)])
    assert values.size == 255 * 7 + 6 + (1 << 20)
    got = _np(itw.srgb_encode_device(_dev(gpu, values)))
    torch.cuda.synchronize()
    want = S.encode(values)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, [(float(values[i]), int(got[i]), int(want[i])) for i in bad[:6]])
    near = values[:255 * 7].reshape(255, 7)
    assert np.array_equal(S.encode(near[:, 3]), np.arange(1, 256)) and np.array_equal(S.encode(near[:, 2]), np.arange(0, 255))     # at T[k]: up; one below: not


@functools.lru_cache(maxsize=None)
def _random_bases(w, h, items):
    return tuple(np.random.default_rng(1000 * w + 10 * h + i).integers(0, 256, (h, w, 4), dtype=np.uint8) for i in range(items))


@functools.lru_cache(maxsize=None)
def _model(w, h, items):
    return tuple(tuple(S.chain(b)) for b in _random_bases(w, h, items))


def _canvas_chain(w, h, items, device):
    """Every level of every item a strided view inside ONE pattern-filled canvas, three pattern rows and a few pattern texels around each;
    rows start 3 texels past a 16-byte boundary.  Returns (canvas, chains of views, first row of every view, the pattern)."""
    n = M.levels_of(w, h)
    pitch = (3 + w + 5) * 4
    pitch += (-pitch) % 16
    rows = 3 + items * sum(max(1, h >> l) + 3 for l in range(n))
    pattern = G.pattern(rows * pitch).reshape(rows, pitch)
    if device is None:
        canvas = pattern.copy()
    else:
        import torch
        canvas = torch.from_numpy(pattern.copy()).to(device)
    chains, tops, y = [], [], 3
    for _ in range(items):
        ch, top = [], []
        for l in range(n):
            lw, lh = M.level_size(w, h, l)
            sub = canvas[y:y + lh, 12:(3 + lw) * 4]
            ch.append(np.lib.stride_tricks.as_strided(sub, (lh, lw, 4), (sub.strides[0], 4, 1)) if device is None else sub.unflatten(1, (lw, 4)))
            top.append(y)
            y += lh + 3
        chains.append(ch)
        tops.append(top)
    return canvas, chains, tops, pattern


def _run_in_canvas(itw, gpu, w, h, items, where, per_level):
    """The canvas after the call is the pattern with the bases and the model's levels in their places, byte for byte: level 0 is not
    written, and neither is anything outside width x height of a written level."""
    import torch
    bases, want = _random_bases(w, h, items), _model(w, h, items)
    canvas, chains, tops, pattern = _canvas_chain(w, h, items, gpu if where == "device" else None)
    expected = pattern.copy()
    for ch, top, b, model in zip(chains, tops, bases, want):
        if where == "device":
            ch[0].copy_(_dev(gpu, b))
        else:
            ch[0][...] = b
        for lv, y in zip(model, top):
            expected[y:y + lv.shape[0], 12:(3 + lv.shape[1]) * 4] = lv.reshape(lv.shape[0], lv.shape[1] * 4)
    itw.generate_mips_into(chains, per_level=per_level, srgb=True)
    torch.cuda.synchronize()
    after = _np(canvas)
    bad = np.argwhere(after != expected)
    assert bad.size == 0, (w, h, items, where, per_level, len(bad), bad[:4].tolist())
    return after


# 2 x 2; 64^2: one pyramid tile; 128^2: pyramid, then the tail; 128 x 32 and 512 x 2: the per-level bridge; 64 x 256; 1 x 8; six items of 64^2
BOX_CASES = [(2, 2, 1), (64, 64, 1), (128, 128, 1), (128, 32, 1), (512, 2, 1), (64, 256, 1), (1, 8, 1), (64, 64, 6)]      # (width, height, items)


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("w,h,items", BOX_CASES)
def test_box_chains_on_both_routes_inside_a_guarded_canvas(itw, gpu, w, h, items, where):
    routes = [_run_in_canvas(itw, gpu, w, h, items, where, per_level) for per_level in (False, True)]
    assert np.array_equal(routes[0], routes[1])
    plain = [M.chain(b) for b in _random_bases(w, h, items)]
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(_model(w, h, items), plain)), "the flag changed nothing: the case shows nothing"


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("w,h", [(5, 3), (7, 7), (100, 36)])
def test_linear_chains_inside_a_guarded_canvas(itw, gpu, w, h, where):
    a = _run_in_canvas(itw, gpu, w, h, 2, where, False)
    b = _run_in_canvas(itw, gpu, w, h, 2, where, True)          # the route flag changes nothing for a linear chain
    assert np.array_equal(a, b)


def test_the_256_constants_keep_their_code_at_every_level(itw, gpu):
    """A 64 x 16384 image of 256 tiles of 64 x 64, tile c of code c in all four channels: levels 1 .. 6 hold each tile's code on both routes
    (the pyramid kernel's registers and LDS, the per-level kernel); below that the tiles mix, and the whole chain is the model's.  And 256
    items of 4 x 4 through the tail kernel alone."""
    import torch
    img = np.repeat(np.arange(256, dtype=np.uint8), 64 * 64 * 4).reshape(256 * 64, 64, 4)
    want = S.chain(img)
    for l in range(1, 7):
        assert np.array_equal(want[l], np.repeat(np.arange(256, dtype=np.uint8), (64 >> l) ** 2 * 4).reshape(256 * (64 >> l), 64 >> l, 4)), l
    for per_level in (False, True):
        got = itw.generate_mips(_dev(gpu, img), per_level=per_level, srgb=True)
        torch.cuda.synchronize()
        for l, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(_np(g), w), (per_level, l)
    small = [np.full((4, 4, 4), c, dtype=np.uint8) for c in range(256)]
    for per_level in (False, True):
        got = itw.generate_mips([_dev(gpu, b) for b in small], per_level=per_level, srgb=True)
        torch.cuda.synchronize()
        for c, ch in enumerate(got):
            assert all((_np(lv) == c).all() for lv in ch), (per_level, c)


def test_the_checkerboard_is_188_where_the_plain_rule_gives_128(itw, gpu):
    import torch
    y, x = np.mgrid[0:64, 0:64]
    img = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 4, axis=2)
    for per_level in (False, True):
        got = [_np(lv) for lv in itw.generate_mips(_dev(gpu, img), per_level=per_level, srgb=True)]
        plain = [_np(lv) for lv in itw.generate_mips(_dev(gpu, img), per_level=per_level)]
        torch.cuda.synchronize()
        assert (got[1][..., :3] == 188).all() and (got[1][..., 3] == 128).all() and (plain[1] == 128).all()
        for g, w in zip(got, S.chain(img)):
            assert np.array_equal(g, w)
        assert all(np.array_equal(g[..., 3], p[..., 3]) for g, p in zip(got, plain))          # alpha follows the old rule at every level
    host = itw.generate_mips(img, srgb=True)
    assert all(np.array_equal(g, w) for g, w in zip(host, S.chain(img)))


def _mipped_ex(itw, fmt, bases, flags, settings):
    """itwCompressImageMippedEx as a caller writes it: (ok, blocks as a numpy array)."""
    import torch
    h, w = bases[0].shape[:2]
    n = itw.mip_levels(w, h)
    base = fmt.split("_")[0]
    nbytes = len(bases) * sum(((max(1, w >> l) + 3) // 4) * ((max(1, h >> l) + 3) // 4) for l in range(n)) * itw.BYTES_PER_BLOCK[base]
    on_device = hasattr(bases[0], "data_ptr")
    out = torch.zeros(nbytes, dtype=torch.uint8, device=bases[0].device) if on_device else np.zeros(nbytes, dtype=np.uint8)
    if on_device:
        itw.lib().itwSetStream(torch.cuda.current_stream(bases[0].device).cuda_stream)
    sp = C.cast(C.byref(settings), C.c_void_p) if settings is not None else None
    ok = itw.lib().itwCompressImageMippedEx(C.cast(itw.abi._surfaces(bases), C.c_void_p), len(bases), 0, 0, flags,
                                            out.data_ptr() if on_device else out.ctypes.data, itw.DXGI_FORMAT[fmt], sp, None, None)
    torch.cuda.synchronize()
    return bool(ok), _np(out)


@pytest.mark.parametrize("case", ["64^2 cube as BC1", "37x29 as BC7 veryfast"])
def test_the_one_call_save_is_generate_then_the_chain_call(itw, gpu, case):
    import torch
    if case.startswith("64"):
        fmt, settings, bases = "bc1_srgb", None, [np.random.default_rng(300 + f).integers(0, 256, (64, 64, 4), dtype=np.uint8) for f in range(6)]
        src = [_dev(gpu, b) for b in bases]
    else:
        fmt, settings, bases = "bc7_srgb", itw.bc7_profile("veryfast"), [np.random.default_rng(310).integers(0, 256, (29, 37, 4), dtype=np.uint8)]
        src = [b.copy() for b in bases]
    ok, got = _mipped_ex(itw, fmt, src, itw.MIP_SRGB, settings)
    assert ok, itw.last_error()
    assert all(np.array_equal(_np(s), b) for s, b in zip(src, bases)), "a base was written"
    chains = itw.generate_mips([_dev(gpu, b) for b in bases], srgb=True)
    for ch, b in zip(chains, bases):
        assert all(np.array_equal(_np(g), w) for g, w in zip(ch, S.chain(b)))
    ok, want = itw.compress_chain(fmt, [lv for ch in chains for lv in ch], settings=settings)
    torch.cuda.synchronize()
    assert ok and np.array_equal(got, _np(want)), case
    ok, bound = itw.compress_mipped(fmt, src, settings=settings, srgb=True)                   # the binding's spelling of the same call
    torch.cuda.synchronize()
    assert ok and np.array_equal(_np(bound), got)
    # flags 0: itwCompressImageMipped's bytes, and the format code alone asks for nothing
    ok, plain_ex = _mipped_ex(itw, fmt, src, 0, settings)
    ok2, plain = itw.compress_mipped(fmt, src, settings=settings)
    torch.cuda.synchronize()
    assert ok and ok2 and np.array_equal(plain_ex, _np(plain)) and not np.array_equal(plain_ex, got)
    ok, per_level = _mipped_ex(itw, fmt, src, itw.MIP_SRGB | itw.MIP_PER_LEVEL, settings)
    assert ok and np.array_equal(per_level, got)
