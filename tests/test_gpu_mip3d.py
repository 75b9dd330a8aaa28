"""itwGenerateMipChain with ITW_MIP_VOLUME on the device (include/itw_dispatch.h, "Mip chains: volumes"; csrc/mip3d.hip).  Every comparison is == on bytes:
RGBA16F against the reference's own functions as tests/golden/mip3d_ref.npz and mip3d_ref_sha256.json record them, RGBA8 and RGBA8 with
sRGB colour against the numpy model of tests/_mip3d.py, which tests/test_mip3d_cpu.py pins to that recording."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import _guarded as G
import _mip3d as M3
import _mipgen as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLD, "mip3d_ref_sha256.json")) as _f:
    PINS = json.load(_f)["cases"]
# beside the recorded sizes: two x tiles of a level (65 texels), three y tiles (9 rows), an odd depth
WIDE = (130, 19, 5, 91)


@pytest.fixture(scope="module")
def arrays():
    return dict(np.load(os.path.join(GOLD, "mip3d_ref.npz")))


def _dev(gpu, a):
    import torch
    a = a.copy()                                                   # (the shared bases are read-only)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(gpu)


def _np(t, dtype):
    return (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)).view(dtype)


@functools.lru_cache(maxsize=None)
def _base(kind, w, h, d, seed):
    b = M3.seeded_half_volume(d, h, w, seed) if kind == "rgba16f" else M3.seeded_byte_volume(d, h, w, seed)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _model(kind, w, h, d, seed, filt, wrap):
    """The model's chain, computed once and shared; read-only."""
    out = M3.chain(_base(kind, w, h, d, seed), filt, wrap, kind)
    for lv in out:
        lv.setflags(write=False)
    return out


def _run(itw, gpu, base, filt, wrap, kind, where="device", **more):
    import torch
    vol = _dev(gpu, base) if where == "device" else base.copy()
    got = itw.generate_mips_3d(vol, filter=None if filt == "box" else filt, wrap=wrap, srgb=kind == "srgb", **more)
    torch.cuda.synchronize()
    return got


def _equal_chain(got, want, what):
    assert len(got) == len(want), what
    for l, (g, w) in enumerate(zip(got, want)):
        g = _np(g, w.dtype)
        assert g.shape == w.shape, (what, l, g.shape, w.shape)
        bad = np.argwhere((g != w).any(axis=3))
        assert bad.size == 0, (what, f"level {l}: {len(bad)} texels differ, first at (z, y, x) = {bad[0].tolist()}: "
                               f"got {g[tuple(bad[0])].tolist()} want {w[tuple(bad[0])].tolist()}")


def _all_cases():
    for c in M3.CASES + M3.SHA_CASES:
        yield c, M3.variants(*c[:3])
    for c in M3.WIDE_BOX_CASES:
        yield c, [("box", "")]


@pytest.mark.parametrize("filt", M3.FILTERS)
def test_rgba16f_equals_the_recorded_reference(itw, gpu, arrays, filt):
    """every recorded case, the three hash-only ones among them; `box` is the default filter of a power-of-two volume"""
    seen = 0
    for (w, h, d, seed), vs in _all_cases():
        base = _base("rgba16f", w, h, d, seed)
        for f, wrap in vs:
            if f != filt:
                continue
            name = M3.case_name(f, wrap, w, h, d)
            e = PINS[name]
            assert hashlib.sha256(base.tobytes()).hexdigest() == e["input_sha256"], name
            levels = [_np(g, np.uint16) for g in _run(itw, gpu, base, f, wrap, "rgba16f")]
            if e["stored"]:
                for l in e["levels"]:
                    _equal_chain([levels[l]], [arrays[f"{name}_l{l}"]], (name, l))
            assert hashlib.sha256(b"".join(np.ascontiguousarray(levels[l]).tobytes() for l in e["levels"])).hexdigest() == e["levels_sha256"], name
            seen += 1
    assert seen == {"box": 14, "point": 18, "linear": 18, "cubic": 54, "triangle": 54}[filt]


@pytest.mark.parametrize("kind", ["rgba8", "srgb"])
@pytest.mark.parametrize("filt", M3.FILTERS)
def test_rgba8_and_srgb_equal_the_model(itw, gpu, filt, kind):
    """every stored case, the levels below the reference's stale scanline included: there the model's rule is the library's"""
    for (w, h, d, seed), vs in list(_all_cases()) + [(WIDE, M3.variants(*WIDE[:3]))]:
        if (w, h, d, seed) in M3.SHA_CASES:
            continue
        for f, wrap in vs:
            if f == filt:
                _equal_chain(_run(itw, gpu, _base(kind, w, h, d, seed), f, wrap, kind), _model(kind, w, h, d, seed, f, wrap), (f, wrap, kind, (w, h, d)))


@pytest.mark.parametrize("kind", M3.KINDS)
def test_host_pointers_equal_device_pointers_and_the_model(itw, gpu, kind):
    for w, h, d, seed in ((12, 20, 6, 83), (16, 16, 16, 79), (1, 1, 8, 77), (16, 4, 16, 90), WIDE):
        for f, wrap in M3.variants(w, h, d):
            if wrap in ("", "uvw"):
                want = _model(kind, w, h, d, seed, f, wrap)
                host = _run(itw, gpu, want[0], f, wrap, kind, "host")
                assert host[0].tobytes() == want[0].tobytes()
                _equal_chain(host, want, (f, wrap, kind, "host"))
                _equal_chain(_run(itw, gpu, want[0], f, wrap, kind, "device"), want, (f, wrap, kind, "device"))
    # fewer levels than the full chain
    want = _model(kind, 12, 20, 6, 83, "cubic", "w")
    got = itw.generate_mips_3d(want[0].copy(), levels=3, filter="cubic", wrap="w", srgb=kind == "srgb")
    _equal_chain(got, want[:3], (kind, "three levels"))


def test_the_default_is_triangle_for_other_sizes_and_per_level_changes_nothing(itw, gpu):
    for kind in M3.KINDS:
        for w, h, d, seed in ((12, 20, 6, 83), (5, 3, 7, 80), (16, 16, 16, 79), (12, 20, 1, 85)):
            named = "box" if M3.default_filter(w, h, d) == "box" else "triangle"
            want = _model(kind, w, h, d, seed, named, "")
            _equal_chain(_run(itw, gpu, want[0], None, "", kind), want, (kind, (w, h, d), "default"))
            _equal_chain(_run(itw, gpu, want[0], None, "", kind, per_level=True), want, (kind, (w, h, d), "per level"))
            if named == "triangle":
                _equal_chain(_run(itw, gpu, want[0], "triangle", "", kind, per_level=True), want, (kind, (w, h, d), "named"))


def test_the_wrap_bits_leave_box_point_and_linear_unchanged(itw, gpu):
    for kind in M3.KINDS:
        for w, h, d, seed in ((16, 16, 16, 79), (12, 20, 6, 83), (4, 8, 2, 74), (1, 8, 1, 78)):
            for f in ("box", "point", "linear"):
                if f == "box" and M3.default_filter(w, h, d) != "box":
                    continue
                want = _model(kind, w, h, d, seed, f, "")
                for wrap in ("u", "w", "uvw"):
                    _equal_chain(_run(itw, gpu, want[0], f, wrap, kind), want, (kind, f, wrap, (w, h, d)))


@pytest.mark.parametrize("kind", M3.KINDS)
def test_a_depth_of_one_writes_the_2d_calls_bytes(itw, gpu, kind):
    """itwGenerateMipChain's bytes for the same explicit filter: box as the 2D default of a power-of-two image, cubic and triangle by
    their bits, point and linear through the free-size chain at the definition's sizes.  Triangle too: the recorded 12x20x1 case is the
    2D recording's, and the z list of 1 -> 1 has the one weight 1.0f (tests/test_mip3d_cpu.py)."""
    import torch
    for w, h, seed in ((12, 20, 85), (8, 8, 84), (64, 2, 92)):
        vol = _base(kind, w, h, 1, seed)
        filters = ("point", "linear", "cubic", "triangle") + (("box",) if M.is_pow2(w) and M.is_pow2(h) else ())
        for f in filters:
            for wrap in (("", "uv") if f in ("cubic", "triangle") else ("",)):
                got = _run(itw, gpu, vol, f, wrap, kind)
                img = _dev(gpu, vol[0])
                if f in ("point", "linear"):
                    flat = [img] + [torch.zeros((g.shape[1], g.shape[2], 4), dtype=img.dtype, device=gpu) for g in got[1:]]
                    itw.resize_chain_into([flat], filter=f, srgb=kind == "srgb")
                else:
                    flat = itw.generate_mips(img, filter=None if f == "box" else f, wrap=wrap, srgb=kind == "srgb")
                torch.cuda.synchronize()
                assert len(flat) == len(got)
                for l in range(1, len(got)):
                    assert np.array_equal(_np(got[l], vol.dtype)[0], _np(flat[l], vol.dtype)), (kind, (w, h), f, wrap, l)


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("kind", M3.KINDS)
def test_slices_as_views_of_a_guarded_canvas(itw, gpu, kind, where):
    """Every slice of every level is a strided view inside one guarded allocation, pattern rows and texels around each, rows 3 texels
    past a 16-byte boundary.  After the call the payload is what it was with the model's levels in their places, and both guards hold:
    level 0 is not written, and neither is anything outside width x height of a written slice."""
    import torch
    w, h, d, seed = 21, 10, 6, 93
    sizes = [M3.level_size(w, h, d, l) for l in range(M3.levels_of(w, h, d))]
    isz = _base(kind, 1, 1, 1, 0).itemsize
    px = 4 * isz
    pitch = (3 + w + 5) * px
    pitch += (-pitch) % 16
    rows = 3 + sum(ld * (lh + 2) for _, lh, ld in sizes)
    for filt, wrap in ((None, ""), ("point", ""), ("linear", "w"), ("cubic", "uvw"), ("triangle", "w")):
        g = G.guarded(rows * pitch, device=gpu if where == "device" else None)
        if where == "device":
            texels = (g.view.view(torch.int16) if isz == 2 else g.view).reshape(rows, pitch // isz)
        else:
            texels = g.view.view(_base(kind, 1, 1, 1, 0).dtype).reshape(rows, pitch // isz)
        levels, places, y = [], [], 3
        for lw, lh, ld in sizes:
            sl, top = [], []
            for _ in range(ld):
                sub = texels[y:y + lh, 12:(3 + lw) * 4]
                sl.append(np.lib.stride_tricks.as_strided(sub, (lh, lw, 4), (sub.strides[0], 4 * isz, isz)) if where == "host" else sub.unflatten(1, (lw, 4)))
                top.append(y)
                y += lh + 2
            levels.append(sl)
            places.append(top)
        base = _base(kind, w, h, d, seed)
        for z, s in enumerate(levels[0]):
            if where == "device":
                s.copy_(_dev(gpu, base[z]))
            else:
                s[...] = base[z]
        expected = g.host().copy().reshape(rows, pitch)
        for lv, top in zip(_model(kind, w, h, d, seed, filt or "triangle", wrap), places):
            for z, y in enumerate(top):
                expected[y:y + lv.shape[1], 3 * px:(3 + lv.shape[2]) * px] = lv[z].view(np.uint8).reshape(lv.shape[1], lv.shape[2] * px)
        itw.generate_mips_3d_into(levels, filter=filt, wrap=wrap, srgb=kind == "srgb")
        torch.cuda.synchronize()
        g.check((filt, kind, where))
        bad = np.argwhere(g.host().reshape(rows, pitch) != expected)
        assert bad.size == 0, (filt, kind, where, len(bad), bad[:4].tolist())


def test_two_volumes_of_one_base_size_and_two_wraps_back_to_back(itw, gpu):
    """the triangle lists are cached by wrap bits, level count and base size: a second call with another key must not run the first's"""
    for kind in ("rgba16f", "rgba8"):
        for (w, h, d, seed), wrap, levels in (((12, 20, 6, 83), "", 0), ((12, 20, 6, 83), "w", 0), ((12, 20, 6, 83), "w", 3), ((12, 6, 20, 94), "w", 3), ((12, 20, 6, 83), "", 0)):
            want = _model(kind, w, h, d, seed, "triangle", wrap)
            n = levels or len(want)
            for where in ("device", "host"):
                vol = _dev(gpu, want[0]) if where == "device" else want[0].copy()
                _equal_chain(itw.generate_mips_3d(vol, levels=levels, filter="triangle", wrap=wrap), want[:n], (kind, (w, h, d), wrap, levels, where))
