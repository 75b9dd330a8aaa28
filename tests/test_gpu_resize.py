"""ITW_MIP_RESIZE on the device (include/itw_dispatch.h, "Mip chains: free sizes"; csrc/resize.hip).  Every comparison is == on bytes:
RGBA16F against the reference's own functions as tests/golden/resize_ref.npz and resize_ref_sha256.json record them, RGBA8 and RGBA8 with
sRGB colour against the numpy model of tests/_resize.py, which tests/test_resize_cpu.py pins to that recording."""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import _guarded as G
import _mip_filters as MF
import _resize as R
import _stream_order as so

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLD, "resize_ref_sha256.json")) as _f:
    PINS = json.load(_f)["cases"]
SMALL = 4096
# the cases RGBA8 and sRGB run as well: every one whose levels are all stored (the model of the others is the CPU suite's business)
STORED_CASES = [(sizes, seed) for sizes, seed in R.CASES if all(w * h <= SMALL for w, h in sizes)]
LONG_LISTS = [((64, 64), (16, 16)), ((130, 70), (3, 2)), ((100, 36), (17, 64))]


@pytest.fixture(scope="module")
def arrays():
    return dict(np.load(os.path.join(GOLD, "resize_ref.npz")))


def _dev(gpu, a):
    import torch
    a = a.copy()                                                   # (the shared bases are read-only)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(gpu)


def _np(t, dtype):
    return (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)).view(dtype)


@functools.lru_cache(maxsize=None)
def _base(kind, w, h, seed):
    b = MF.seeded_half_image(h, w, seed) if kind == "rgba16f" else MF.seeded_byte_image(h, w, seed)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _model(kind, sizes, seed, filt, addr):
    """The model's chain, computed once and shared; read-only."""
    out = R.chain(_base(kind, sizes[0][0], sizes[0][1], seed), sizes, filt, addr, kind)
    for lv in out:
        lv.setflags(write=False)
    return out


def _options(addr):
    return dict(wrap="" if addr == "mirror" else addr, mirror="uv" if addr == "mirror" else "")


def _run(itw, gpu, base, sizes, filt, addr, kind, where="device", lib=None):
    """the chain [base, level 1, ...] through resize_chain_into (or library instance `lib`) from device or host pointers"""
    import torch
    if where == "device":
        b = _dev(gpu, base)
        chain = [b] + [torch.zeros((h, w, 4), dtype=b.dtype, device=gpu) for w, h in sizes[1:]]
    else:
        chain = [base.copy()] + [np.zeros((h, w, 4), dtype=base.dtype) for w, h in sizes[1:]]
    if lib is None:
        itw.resize_chain_into([chain], filter=None if filt == "box" else filt, srgb=kind == "srgb", **_options(addr))
    else:
        lib.itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
        flags = itw.resize_flags(None if filt == "box" else filt, srgb=kind == "srgb", **_options(addr))
        assert lib.itwGenerateMipChain(C.cast(itw.abi._surfaces(chain), C.c_void_p), 1, len(chain), 4 * base.itemsize, flags) == 0, itw.last_error()
    torch.cuda.synchronize()
    return chain


def _equal_chain(got, want, what):
    assert len(got) == len(want), what
    for l, (g, w) in enumerate(zip(got, want)):
        g = _np(g, w.dtype)
        assert g.shape == w.shape, (what, l, g.shape, w.shape)
        bad = np.flatnonzero((g != w).any(axis=2))
        assert bad.size == 0, (what, f"level {l}: {bad.size} texels differ, first at {divmod(int(bad[0]), w.shape[1])}: "
                               f"got {g.reshape(-1, 4)[bad[0]].tolist()} want {w.reshape(-1, 4)[bad[0]].tolist()}")


@pytest.mark.parametrize("filt", R.FILTERS)
def test_rgba16f_equals_the_recorded_reference(itw, gpu, arrays, filt):
    """every recorded case, the two hash-only ones and the three-level chain among them; `box` is the default filter at exactly 2:1"""
    seen = 0
    for sizes, seed in R.CASES:
        base = _base("rgba16f", sizes[0][0], sizes[0][1], seed)
        for f, addr in R.variants(sizes):
            if f != filt:
                continue
            name = R.case_name(f, addr, sizes)
            e = PINS[name]
            assert hashlib.sha256(base.tobytes()).hexdigest() == e["input_sha256"], name
            levels = [_np(g, np.uint16) for g in _run(itw, gpu, base, sizes, f, addr, "rgba16f")[1:]]
            for i, lv in enumerate(levels):
                if e["stored"][i]:
                    _equal_chain([lv], [arrays[f"{name}_l{i + 1}"]], (name, i + 1))
            assert hashlib.sha256(b"".join(np.ascontiguousarray(lv).tobytes() for lv in levels)).hexdigest() == e["levels_sha256"], name
            seen += 1
    assert seen == {"point": 56, "box": 4, "linear": 37, "cubic": 70, "triangle": 56}[filt]


@pytest.mark.parametrize("kind", ["rgba8", "srgb"])
@pytest.mark.parametrize("filt", R.FILTERS)
def test_rgba8_and_srgb_equal_the_model(itw, gpu, filt, kind):
    for sizes, seed in STORED_CASES:
        base = _base(kind, sizes[0][0], sizes[0][1], seed)
        for f, addr in R.variants(sizes):
            if f == filt:
                _equal_chain(_run(itw, gpu, base, sizes, f, addr, kind), _model(kind, sizes, seed, f, addr), (f, addr, kind, sizes))


def test_the_default_filter_and_host_pointers(itw, gpu, arrays):
    """no filter bit: box at exactly 2:1, linear elsewhere, per level pair; and every filter from host pointers"""
    for sizes, name in ((((16, 16), (8, 8)), "box"), (((7, 7), (3, 3)), "linear"), (((20, 12), (33, 7), (8, 8)), "linear")):
        seed = dict((R.sizes_name(s), k) for s, k in R.CASES)[R.sizes_name(sizes)]
        base = _base("rgba16f", sizes[0][0], sizes[0][1], seed)
        for where in ("device", "host"):
            got = _run(itw, gpu, base, sizes, None, "", "rgba16f", where)
            for i, lv in enumerate(got[1:]):
                _equal_chain([lv], [arrays[f"{R.case_name(name, '', sizes)}_l{i + 1}"]], (sizes, where, i + 1))
    mixed = (((16, 16), (8, 8), (5, 8), (10, 16), (5, 8)), 7)      # box, linear, linear up, box again
    for kind in R.KINDS:
        want = _model(kind, mixed[0], mixed[1], None, "")
        _equal_chain(_run(itw, gpu, want[0], mixed[0], None, "", kind, "host"), want, ("mixed", kind))
    sizes, seed = ((100, 36), (17, 64)), 70
    for kind in R.KINDS:
        base = _base(kind, 100, 36, seed)
        # (linear wraps along x, the axis that shrinks; along y, which grows, the call refuses it)
        for filt, addr in (("point", ""), ("linear", "u"), ("cubic", "mirror"), ("cubic", "uv"), ("triangle", "uv"), ("triangle", "")):
            _equal_chain(_run(itw, gpu, base, sizes, filt, addr, kind, "host"), _model(kind, sizes, seed, filt, addr), (filt, addr, kind, "host"))


@pytest.mark.parametrize("kind", R.KINDS)
def test_the_triangle_filter_with_long_lists(itw, gpu, kind):
    """above the gather's six-entry path, where its general loop runs: 4:1, about 43:1, a mixed pair, a wide source over two tile
    columns and three tile rows, and long lists along y alone; under every wrap"""
    cases = [(s, dict((R.sizes_name(x), k) for x, k in R.CASES)[R.sizes_name(s)]) for s in LONG_LISTS] + [(((1300, 40), (70, 9)), 75), (((300, 150), (130, 11)), 76)]
    for sizes, seed in cases:
        base = _base(kind, sizes[0][0], sizes[0][1], seed)
        for addr in MF.WRAPS:
            _equal_chain(_run(itw, gpu, base, sizes, "triangle", addr, kind), _model(kind, sizes, seed, "triangle", addr), (sizes, addr, kind))


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_two_items_as_views_of_a_guarded_canvas(itw, gpu, kind, where):
    """Both items' levels are strided views inside one guarded allocation, pattern rows and texels around each, rows 3 texels past a
    16-byte boundary.  After the call the payload is what it was with the model's levels in their places, and both guards hold: level 0
    is not written, and neither is anything outside width x height of a written level."""
    import torch
    sizes, items = ((33, 9), (70, 21), (5, 30)), 2
    isz = _base(kind, 1, 1, 0).itemsize
    px = 4 * isz
    pitch = (3 + max(w for w, _ in sizes) + 5) * px
    pitch += (-pitch) % 16
    rows = 3 + items * sum(h + 3 for _, h in sizes)
    for filt, addr in (("point", ""), (None, ""), ("cubic", "mirror"), ("triangle", "v")):
        g = G.guarded(rows * pitch, device=gpu if where == "device" else None)
        if where == "device":
            texels = (g.view.view(torch.int16) if isz == 2 else g.view).reshape(rows, pitch // isz)
        else:
            texels = g.view.view(_base(kind, 1, 1, 0).dtype).reshape(rows, pitch // isz)
        chains, places, y = [], [], 3
        for _ in range(items):
            ch, top = [], []
            for lw, lh in sizes:
                sub = texels[y:y + lh, 12:(3 + lw) * 4]
                ch.append(np.lib.stride_tricks.as_strided(sub, (lh, lw, 4), (sub.strides[0], 4 * isz, isz)) if where == "host" else sub.unflatten(1, (lw, 4)))
                top.append(y)
                y += lh + 3
            chains.append(ch)
            places.append(top)
        for s, ch in enumerate(chains):
            b = _base(kind, sizes[0][0], sizes[0][1], 80 + s)
            if where == "device":
                ch[0].copy_(_dev(gpu, b))
            else:
                ch[0][...] = b
        expected = g.host().copy().reshape(rows, pitch)
        for s, top in enumerate(places):
            for lv, y in zip(_model(kind, sizes, 80 + s, filt, addr), top):
                expected[y:y + lv.shape[0], 3 * px:(3 + lv.shape[1]) * px] = lv.view(np.uint8).reshape(lv.shape[0], lv.shape[1] * px)
        itw.resize_chain_into(chains, filter=filt, srgb=kind == "srgb", **_options(addr))
        torch.cuda.synchronize()
        g.check((filt, kind, where))
        bad = np.argwhere(g.host().reshape(rows, pitch) != expected)
        assert bad.size == 0, (filt, kind, where, len(bad), bad[:4].tolist())


def test_two_resizes_of_one_base_to_two_targets_back_to_back(itw, gpu):
    """one base, one chain length, two targets: the triangle lists' cache key holds every level's size, or the second call runs the first's"""
    for kind in ("rgba16f", "rgba8"):
        base = _base(kind, 64, 64, 68)
        for filt in ("triangle", "cubic", None):
            for where in ("device", "host"):
                for target in ((16, 16), (24, 16), (16, 16), (16, 40), (24, 16)):
                    sizes = ((64, 64), target)
                    _equal_chain(_run(itw, gpu, base, sizes, filt, "", kind, where), _model(kind, sizes, 68, filt, ""), (kind, filt, where, target))
        # and an ordinary chain of the same base and length between them
        got = itw.generate_mips(_dev(gpu, base), levels=2, filter="triangle")
        _equal_chain(got, MF.chain(base, "triangle", "", kind, levels=2), (kind, "ordinary chain after a resize"))
        _equal_chain(_run(itw, gpu, base, ((64, 64), (32, 33)), "triangle", "", kind), _model(kind, ((64, 64), (32, 33)), 68, "triangle", ""), (kind, "after it"))


def test_the_python_resize_call(itw, gpu):
    import torch
    base = _base("rgba8", 20, 12, 74)
    want = _model("rgba8", ((20, 12), (33, 7)), 74, "cubic", "")[1]
    got = itw.resize(_dev(gpu, base), size=(33, 7), filter="cubic")
    torch.cuda.synchronize()
    assert np.array_equal(_np(got, np.uint8), want) and np.array_equal(itw.resize(base.copy(), size=(33, 7), filter="cubic"), want)
    both = itw.resize([base.copy(), base.copy()], fit="pow2")
    assert [b.shape for b in both] == [(8, 16, 4)] * 2 and np.array_equal(both[0], R.level(base, (16, 8), None, "", "rgba8")) and np.array_equal(both[0], both[1])
    out = np.zeros((16, 32, 4), np.uint8)
    assert itw.resize(base.copy(), fit="pow2_up", filter="linear", out=out) is out and np.array_equal(out, R.level(base, (32, 16), "linear", "", "rgba8"))
    srgb = itw.resize(base.copy(), fit="multiple4", filter="triangle", srgb=True, wrap="uv")
    assert np.array_equal(srgb, R.level(base, (20, 12), "triangle", "uv", "srgb"))
    with pytest.raises(ValueError):
        itw.resize(base.copy())
    itw.set_error_mode(itw.ON_ERROR_RETURN)
    try:
        with pytest.raises(ValueError, match="linear filter with ITW_MIP_WRAP"):
            itw.resize(base.copy(), size=(40, 12), wrap="u")
        assert "ITW_MIP_CUBIC and ITW_MIP_TRIANGLE" in itw.last_error()
    finally:
        itw.lib().itwClearError()
        itw.set_error_mode(itw.ON_ERROR_ABORT)


def test_compress_mipped_resizes_first(itw, gpu):
    import torch
    base = _base("rgba8", 20, 12, 74)
    for resize, filt in (((16, 8), "triangle"), ("pow2", None)):
        ok, got = itw.compress_mipped("bc1", _dev(gpu, base), resize=resize, resize_filter=filt)
        torch.cuda.synchronize()
        fitted = itw.resize(base.copy(), size=(16, 8), filter=filt)
        ok2, want = itw.compress_mipped("bc1", fitted)
        ok3, host = itw.compress_mipped("bc1", base.copy(), resize=resize, resize_filter=filt)
        assert ok and ok2 and ok3 and np.array_equal(_np(got, np.uint8), want) and np.array_equal(host, want), (resize, filt)


def test_an_inf_and_a_nan_texel_under_point_and_cubic(itw, gpu):
    """point: the texel goes through the store, +-Inf becomes +-65504 and a NaN 0x7E00; cubic: inf - inf in its differences makes NaN"""
    base = MF.seeded_half_image(9, 11, 99).copy()
    base[3, 5] = [0x7C00, 0xFC00, 0x7E01, 0xFFFF]                  # +inf, -inf, two NaNs; a texel the point filter samples at every size below
    base[3, 6] = [0xFC00, 0x3C00, 0x3C00, 0x7C00]
    for sizes in (((11, 9), (23, 17)), ((11, 9), (6, 5)), ((11, 9), (11, 9))):
        want = R.chain(base, sizes, "point", "")
        hit = (want[1] == np.array([0x7BFF, 0xFBFF, 0x7E00, 0x7E00], np.uint16)).all(axis=2)
        assert hit.any() and not (want[1] == 0x7C00).any() and not (want[1] == 0xFC00).any()
        _equal_chain(_run(itw, gpu, base, sizes, "point", "", "rgba16f"), want, ("point", sizes))
        for addr in ("", "mirror", "uv"):
            want = R.chain(base, sizes, "cubic", addr)
            assert (want[1] == 0x7E00).any()
            _equal_chain(_run(itw, gpu, base, sizes, "cubic", addr, "rgba16f"), want, ("cubic", addr, sizes))


def test_an_ordinary_cubic_chain_is_what_it_was_through_both_kernels(itw, gpu):
    """the definition-sized chain's kernels are untouched: ITW_MIP_CUBIC without the resize bit equals tests/_mip_filters.chain"""
    import torch
    T = itw.test_lib()
    base = _base("rgba16f", 130, 70, 5)
    want = MF.chain(base, "cubic", "u")
    try:
        for lds in (1, 0):
            T.itwTestMipCubicVariant(lds)
            b = _dev(gpu, base)
            chain = [b] + [torch.zeros(lv.shape, dtype=b.dtype, device=gpu) for lv in want[1:]]
            T.itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
            assert T.itwGenerateMipChain(C.cast(itw.abi._surfaces(chain), C.c_void_p), 1, len(chain), 8, itw.mip_filter_flags("cubic", "u")) == 0
            torch.cuda.synchronize()
            _equal_chain(chain, want, ("cubic chain", lds))
    finally:
        T.itwTestMipCubicVariant(0)
    _equal_chain(itw.generate_mips(_dev(gpu, base), filter="cubic", wrap="u"), want, "cubic chain, product")


def test_a_resize_keeps_stream_order_with_the_callers_work(itw, gpu):
    """tests/_stream_order.py's device scheme (sequence A) around one free-size chain: the call reads its base after the caller's copy
    into it, its levels are what the caller's next kernel sees, and the caller's later copy into the base does not reach them"""
    import torch
    sizes = ((64, 64), (48, 80), (16, 16))
    contents = [[so._mip_content("half", 64, 64, k)] for k in range(3)]
    wants = [[np.ascontiguousarray(l) for l in R.chain(c[0], sizes, "triangle", "")[1:]] for c in contents]
    shapes = [tuple(l.shape) for l in wants[1]]

    def call(srcs, outs):
        itw.resize_chain_into([[srcs[0]] + [so._as_image(o, torch, s, 2) for o, s in zip(outs, shapes)]], filter="triangle")
    delay = so.Delay(torch, gpu)
    S = torch.cuda.Stream(gpu)
    delay(S)
    torch.cuda.synchronize()
    env = so.Env(itw, None, gpu, torch, delay, S, so.Report())
    try:
        so.run_device("resize-triangle", so.DeviceCase(contents, wants, [8 for _ in shapes], call), env, must_return_early=False)
    finally:
        itw.lib().itwSetStream(None)
        torch.cuda.synchronize()
