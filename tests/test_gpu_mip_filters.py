"""ITW_MIP_CUBIC and ITW_MIP_TRIANGLE on the device (include/itw_dispatch.h, "Mip chains: cubic and triangle"; csrc/mip_filters.hip).
Every comparison is == on bytes: against the reference's own functions where a recorded case exists (tests/golden/mipfilter_ref.npz,
mipfilter_ref_sha256.json), against the numpy model of tests/_mip_filters.py -- which tests/test_mip_filters_cpu.py pins to that recording --
everywhere else.  The cubic filter runs through both of its kernels (the hooks build's itwTestMipCubicVariant)."""
import ctypes as C
import functools
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import _alpha_mips as A
import _guarded as G
import _mip_filters as MF
import _mipgen as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "examples", "encode_dds")
with open(os.path.join(GOLD, "mipfilter_ref_sha256.json")) as _f:
    PINS = json.load(_f)["cases"]

# (width, height): 257 x 17 is one texel past a multiple of the 128 x 8 source texels a workgroup of the LDS cubic kernel stages at 2:1
SIZES = [(2, 2), (1, 8), (8, 1), (3, 5), (7, 7), (12, 20), (64, 64), (65, 33), (130, 70), (256, 4), (4, 256), (256, 256), (257, 17)]
FILTERS = ("cubic", "triangle")


def _dev(gpu, a):
    import torch
    a = a.copy()                                                   # (the shared bases are read-only)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(gpu)


def _np(t, dtype):
    return (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)).view(dtype)


@functools.lru_cache(maxsize=None)
def _base(kind, w, h, seed=0):
    b = MF.seeded_half_image(h, w, 7000 + seed + 3 * w + h) if kind == "rgba16f" else MF.seeded_byte_image(h, w, 7000 + seed + 3 * w + h)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _model(kind, w, h, filt, wrap, seed=0):
    """The model's chain, computed once and shared; read-only."""
    out = MF.chain(_base(kind, w, h, seed), filt, wrap, kind)
    for lv in out:
        lv.setflags(write=False)
    return out


def _equal_chain(got, want, what):
    assert len(got) == len(want), what
    for l, (g, w) in enumerate(zip(got, want)):
        g = _np(g, w.dtype)
        assert g.shape == w.shape, (what, l, g.shape, w.shape)
        bad = np.flatnonzero((g != w).any(axis=2))
        assert bad.size == 0, (what, f"level {l}: {bad.size} texels differ, first at {divmod(int(bad[0]), w.shape[1])}: "
                               f"got {g.reshape(-1, 4)[bad[0]].tolist()} want {w.reshape(-1, 4)[bad[0]].tolist()}")


def _empty_chain(gpu, b):
    import torch
    h, w = b.shape[:2]
    t = _dev(gpu, b)
    return [t] + [torch.zeros((max(1, h >> l), max(1, w >> l), 4), dtype=t.dtype, device=gpu) for l in range(1, M.levels_of(w, h))]


def _raw_generate(L, itw, chains, flags):
    """itwGenerateMipChain of library instance L (the product's or the hooks build's) over device chains."""
    import torch
    flat = [lv for ch in chains for lv in ch]
    L.itwSetStream(torch.cuda.current_stream(flat[0].device).cuda_stream)
    rc = L.itwGenerateMipChain(C.cast(itw.abi._surfaces(flat), C.c_void_p), len(chains), len(chains[0]), 4 * flat[0].element_size(), flags)
    torch.cuda.synchronize()
    return rc


def _flags(itw, kind, filt, wrap):
    return itw.mip_filter_flags(filt, wrap) | (itw.MIP_SRGB if kind == "srgb" else 0)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("kind", MF.KINDS)
@pytest.mark.parametrize("filt", FILTERS)
def test_chains_equal_the_model_from_device_and_host_pointers(itw, gpu, filt, kind, w, h):
    import torch
    base = _base(kind, w, h)
    T = itw.test_lib()
    for wrap in MF.WRAPS:
        want = _model(kind, w, h, filt, wrap)
        got = itw.generate_mips(_dev(gpu, base), srgb=kind == "srgb", filter=filt, wrap=wrap)
        torch.cuda.synchronize()
        _equal_chain(got, want, (filt, kind, w, h, wrap, "device"))
        host = itw.generate_mips(base.copy(), srgb=kind == "srgb", filter=filt, wrap=wrap)
        _equal_chain(host, want, (filt, kind, w, h, wrap, "host"))
        if filt == "cubic":                                        # the kernel the product does not launch, and the product's once more
            try:
                for lds in (1, 0):
                    T.itwTestMipCubicVariant(lds)
                    ch = _empty_chain(gpu, base)
                    assert _raw_generate(T, itw, [ch], _flags(itw, kind, filt, wrap)) == 0
                    _equal_chain(ch, want, (filt, kind, w, h, wrap, "variant", lds))
            finally:
                T.itwTestMipCubicVariant(0)


def test_one_by_one_with_one_level_is_nothing_to_do(itw, gpu):
    for kind, dtype in (("rgba8", np.uint8), ("rgba16f", np.uint16)):
        base = np.full((1, 1, 4), 0x5A, dtype=dtype)
        for filt in FILTERS:
            got = itw.generate_mips(_dev(gpu, base), filter=filt, wrap="uv")
            assert len(got) == 1 and np.array_equal(_np(got[0], dtype), base)
            assert len(itw.generate_mips(base.copy(), levels=1, filter=filt)) == 1


@pytest.mark.parametrize("filt", FILTERS)
def test_the_device_equals_the_recorded_reference(itw, gpu, filt):
    import torch
    arrays = dict(np.load(os.path.join(GOLD, "mipfilter_ref.npz")))
    names = sorted(n for n, e in PINS.items() if e["filter"] == filt)
    assert len(names) == 60
    for name in names:
        e = PINS[name]
        base = MF.seeded_half_image(e["height"], e["width"], e["seed"])
        assert hashlib.sha256(base.tobytes()).hexdigest() == e["input_sha256"], name
        got = itw.generate_mips(_dev(gpu, base), filter=filt, wrap=e["wrap"])
        torch.cuda.synchronize()
        levels = [_np(g, np.uint16) for g in got[1:]]
        if e["stored"]:
            for i, lv in enumerate(levels):
                assert np.array_equal(lv, arrays[f"{name}_l{i + 1}"]), (name, i + 1)
        assert hashlib.sha256(b"".join(np.ascontiguousarray(lv).tobytes() for lv in levels)).hexdigest() == e["levels_sha256"], name


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("kind", MF.KINDS)
@pytest.mark.parametrize("filt", FILTERS)
def test_levels_as_views_of_a_guarded_canvas(itw, gpu, filt, kind, where):
    """Every level of every item is a strided view inside the payload of one guarded allocation, three pattern rows and a few pattern
    texels around each, rows 3 texels past a 16-byte boundary.  The payload after the call is what it was with the model's levels in their
    places, byte for byte, and both guards hold: level 0 is not written, and neither is anything outside width x height of a written level."""
    import torch
    w, h, items, wrap = 65, 33, 2, "uv"
    bases = [_base(kind, w, h, s) for s in range(items)]
    isz = bases[0].itemsize
    px = 4 * isz
    n = M.levels_of(w, h)
    pitch = (3 + w + 5) * px
    pitch += (-pitch) % 16
    rows = 3 + items * sum(max(1, h >> l) + 3 for l in range(n))
    g = G.guarded(rows * pitch, device=gpu if where == "device" else None)
    if where == "device":
        texels = (g.view.view(torch.int16) if isz == 2 else g.view).reshape(rows, pitch // isz)
    else:
        texels = g.view.view(bases[0].dtype).reshape(rows, pitch // isz)
    chains, places, y = [], [], 3
    for _ in range(items):
        ch, top = [], []
        for l in range(n):
            lw, lh = M.level_size(w, h, l)
            sub = texels[y:y + lh, 12:(3 + lw) * 4]
            ch.append(np.lib.stride_tricks.as_strided(sub, (lh, lw, 4), (sub.strides[0], 4 * isz, isz)) if where == "host" else sub.unflatten(1, (lw, 4)))
            top.append(y)
            y += lh + 3
        chains.append(ch)
        places.append(top)
    for ch, b in zip(chains, bases):
        if where == "device":
            ch[0].copy_(_dev(gpu, b))
        else:
            ch[0][...] = b
    expected = g.host().copy().reshape(rows, pitch)
    for s, (top, b) in enumerate(zip(places, bases)):
        for lv, y in zip(_model(kind, w, h, filt, wrap, s), top):
            expected[y:y + lv.shape[0], 3 * px:(3 + lv.shape[1]) * px] = lv.view(np.uint8).reshape(lv.shape[0], lv.shape[1] * px)
    itw.generate_mips_into(chains, srgb=kind == "srgb", filter=filt, wrap=wrap)
    torch.cuda.synchronize()
    g.check((filt, kind, where))
    bad = np.argwhere(g.host().reshape(rows, pitch) != expected)
    assert bad.size == 0, (filt, kind, where, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("filt", FILTERS)
def test_a_cube_of_six_items(itw, gpu, filt):
    import torch
    for kind in MF.KINDS:
        bases = [_base(kind, 64, 64, s) for s in range(6)]
        got = itw.generate_mips([_dev(gpu, b) for b in bases], srgb=kind == "srgb", filter=filt, wrap="u")
        torch.cuda.synchronize()
        for s in range(6):
            _equal_chain(got[s], _model(kind, 64, 64, filt, "u", s), (filt, kind, "face", s))


@pytest.mark.parametrize("filt", FILTERS)
def test_an_inf_texel_stores_the_one_nan_pattern(itw, gpu, filt):
    import torch
    base = MF.seeded_half_image(20, 12, 99).copy()
    base[7, 5] = [0x7C00, 0xFC00, 0x3C00, 0x7C00]                 # cubic: inf - inf in its differences
    base[7, 6] = [0xFC00, 0x3C00, 0x3C00, 0x7C00]                 # triangle: +inf and -inf meet in one sum (channel 0); inf alone stays inf
    want = MF.chain(base, filt, "v")
    assert any((lv == 0x7E00).any() for lv in want[1:])
    got = itw.generate_mips(_dev(gpu, base), filter=filt, wrap="v")
    torch.cuda.synchronize()
    _equal_chain(got, want, (filt, "inf"))


def test_coverage_over_a_cubic_chain_is_the_rule_over_the_models_chain(itw, gpu):
    import torch
    for w, h in ((64, 64), (37, 19)):
        base = A.cutout(h, w, 5)
        for srgb in (False, True):
            plain = MF.chain(base, "cubic", "uv", "srgb" if srgb else "rgba8")
            want, rows = A.apply_coverage(plain, 128)
            got, report = itw.generate_mips(_dev(gpu, base), srgb=srgb, alpha_coverage=128, report=True, filter="cubic", wrap="uv")
            torch.cuda.synchronize()
            _equal_chain(got, want, ("coverage", w, h, srgb))
            assert [(int(r.texels), int(r.covered_plain), int(r.covered), int(r.threshold)) for r in report] == [tuple(int(v) for v in r) for r in rows]


@pytest.mark.parametrize("filt", FILTERS)
def test_per_level_beside_a_filter_bit_gives_the_same_bytes(itw, gpu, filt):
    import torch
    for kind in MF.KINDS:
        got = itw.generate_mips(_dev(gpu, _base(kind, 64, 64)), srgb=kind == "srgb", per_level=True, filter=filt, wrap="uv")
        torch.cuda.synchronize()
        _equal_chain(got, _model(kind, 64, 64, filt, "uv"), (filt, kind, "per_level"))


@pytest.mark.parametrize("fmt", ["bc1", "bc6h"])
@pytest.mark.parametrize("filt", FILTERS)
def test_mipped_with_a_filter_is_generate_then_the_chain_call(itw, gpu, filt, fmt):
    import torch
    kind = "rgba16f" if fmt == "bc6h" else "rgba8"
    settings = (lambda: itw.bc6h_profile("veryfast")) if fmt == "bc6h" else (lambda: None)
    for w, h in ((64, 64), (37, 19)):
        base = _base(kind, w, h)
        ok, got = itw.compress_mipped(fmt, _dev(gpu, base), settings=settings(), filter=filt, wrap="uv")
        torch.cuda.synchronize()
        assert ok, itw.last_error()
        chain = itw.generate_mips(_dev(gpu, base), filter=filt, wrap="uv")
        ok, want = itw.compress_chain(fmt, chain, settings=settings())
        torch.cuda.synchronize()
        ok2, default = itw.compress_mipped(fmt, _dev(gpu, base), settings=settings())
        torch.cuda.synchronize()
        assert ok and ok2 and got.shape == want.shape and np.array_equal(_np(got, np.uint8), _np(want, np.uint8)), (filt, fmt, w, h)
        assert not np.array_equal(_np(got, np.uint8), _np(default, np.uint8)), "the filter bit changed nothing"


def test_encode_dds_with_the_triangle_filter_writes_the_python_routes_payload(itw, gpu, tmp_path):
    img = _base("rgba8", 40, 24)
    raw, out = tmp_path / "in.raw", tmp_path / "out.dds"
    np.ascontiguousarray(img).tofile(raw)
    r = subprocess.run([EXE, "--mips", "--mip-filter", "triangle", "--mip-wrap", "uv", "bc1", "40", "24", str(raw), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    f = np.fromfile(out, dtype=np.uint8)
    d = itw.DdsDesc()
    off = itw.lib().itwDdsReadHeader(f.ctypes.data, f.size, C.byref(d))
    assert off in (128, 148) and (d.width, d.height, d.mip_levels) == (40, 24, 6)
    ok, want = itw.compress_mipped("bc1", img.copy(), filter="triangle", wrap="uv")
    ok2, plain = itw.compress_mipped("bc1", img.copy())
    assert ok and ok2 and f.size == off + want.size and np.array_equal(f[off:], want) and not np.array_equal(want, plain)
