"""The cubic and triangle mip filters without a GPU (include/itw_dispatch.h, "Mip chains: cubic and triangle"): the numpy model of
tests/_mip_filters.py against the reference's own functions as tests/golden/mipfilter_ref.npz records them (tools/make_mipfilter_golden.py),
the library's host tables against the same recording, every new refusal before any device work, the flag constants, the product's
symbol list, and the scratch and spills of csrc/build/mip_filters.o.  Every comparison is == on every byte."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _mip_filters as MF
import _mipgen as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "intel-texture-works-plugin_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden")

# (width, height, seed) and the (source, dest) pairs the recording holds
CASES = [(2, 2, 41), (1, 8, 42), (8, 1, 43), (4, 4, 44), (3, 5, 45), (5, 3, 46), (7, 7, 47), (12, 20, 48), (16, 16, 49), (64, 64, 50), (256, 4, 51),
         (4, 256, 52), (96, 64, 53), (100, 36, 54), (127, 339, 55)]
PAIRS = [(1, 1), (2, 1), (3, 1), (5, 2), (7, 3), (12, 6), (127, 63), (339, 169), (4000, 2000), (3000, 1500), (8191, 4095)]
CUBIC_TABLE = np.dtype([("u", "<i4", 4), ("x", "<f4")])
TRIANGLE_TABLE = np.dtype([("idx", "<i4", 2), ("w", "<f4")])


@pytest.fixture(scope="module")
def recording():
    arrays = dict(np.load(os.path.join(GOLD, "mipfilter_ref.npz")))
    with open(os.path.join(GOLD, "mipfilter_ref_sha256.json")) as f:
        pins = json.load(f)
    return arrays, pins


def _table_bytes(kind, idx, wgt):
    rec = np.zeros(len(wgt), dtype=CUBIC_TABLE if kind == "cubic" else TRIANGLE_TABLE)
    rec["u" if kind == "cubic" else "idx"] = idx
    rec["x" if kind == "cubic" else "w"] = wgt
    return rec.tobytes()


def _table_name(kind, wrap, source, dest):
    return f"{kind}table_{'wrap' if wrap else 'clamp'}_{source}_{dest}"


def test_the_recording_is_complete(recording):
    arrays, pins = recording
    assert len(pins["cases"]) == len(CASES) * 2 * 4 and len(pins["tables"]) == len(PAIRS) * 2 * 2
    for w, h, seed in CASES:
        for kind in ("cubic", "triangle"):
            for wrap in MF.WRAPS:
                e = pins["cases"][f"{kind}_{wrap or 'clamp'}_{w}x{h}"]
                assert (e["width"], e["height"], e["seed"], e["stored"]) == (w, h, seed, w * h <= 1024)


@pytest.mark.parametrize("kind", ["cubic", "triangle"])
def test_the_model_equals_every_recorded_chain(recording, kind):
    arrays, pins = recording
    for w, h, seed in CASES:
        base = MF.seeded_half_image(h, w, seed)
        for wrap in MF.WRAPS:
            name = f"{kind}_{wrap or 'clamp'}_{w}x{h}"
            e = pins["cases"][name]
            assert hashlib.sha256(base.tobytes()).hexdigest() == e["input_sha256"], name
            levels = MF.chain(base, kind, wrap)[1:]
            if e["stored"]:
                assert np.array_equal(arrays[f"in_{w}x{h}"], base)
                for i, lv in enumerate(levels):
                    assert np.array_equal(lv, arrays[f"{name}_l{i + 1}"]), (name, i + 1)
            assert hashlib.sha256(b"".join(lv.tobytes() for lv in levels)).hexdigest() == e["levels_sha256"], name


def test_the_scalar_scatter_and_the_ranked_form_of_the_triangle_model_agree():
    for w, h, seed in ((2, 2, 1), (1, 8, 2), (8, 1, 3), (3, 5, 4), (7, 7, 5), (12, 20, 6), (17, 9, 7)):
        f = M.widen(MF.seeded_half_image(h, w, seed))
        for wrap in MF.WRAPS:
            a, b = MF.triangle_unrounded_scatter(f, "u" in wrap, "v" in wrap), MF.triangle_unrounded(f, "u" in wrap, "v" in wrap)
            assert a.tobytes() == b.tobytes(), (w, h, wrap)


def test_the_model_equals_every_recorded_table(recording):
    arrays, pins = recording
    for source, dest in PAIRS:
        for wrap in (0, 1):
            taps, x = MF.cubic_filter(source, dest, bool(wrap))
            idx, wgt = MF.triangle_table(source, dest, bool(wrap))
            for kind, i, w_ in (("cubic", taps.astype(np.int32), x), ("triangle", idx, wgt)):
                name = _table_name(kind, wrap, source, dest)
                e = pins["tables"][name]
                assert len(w_) == e["entries"], name
                if e["stored"]:
                    assert np.array_equal(i, arrays[name + "_i"]) and w_.tobytes() == arrays[name + "_w"].tobytes(), name
                assert hashlib.sha256(_table_bytes(kind, i, w_)).hexdigest() == e["sha256"], name


def test_the_librarys_host_tables_equal_the_recorded_ones(itw, recording):
    """itwTestMipFilterTable (libispc_texcomp_test.so only): csrc/mip_filters.hpp's builders, the ones the entry points use."""
    arrays, pins = recording
    T = itw.test_lib()
    assert not hasattr(itw.lib(), "itwTestMipFilterTable") and not hasattr(itw.lib(), "itwTestMipCubicVariant")
    for source, dest in PAIRS:
        for wrap in (0, 1):
            for kind, code in (("cubic", 1), ("triangle", 2)):
                name = _table_name(kind, wrap, source, dest)
                cap = dest if kind == "cubic" else 8 * source + 16
                idx = np.full((cap, 4 if kind == "cubic" else 2), -7, dtype=np.int32)
                wgt = np.full(cap, -7.0, dtype=np.float32)
                n = T.itwTestMipFilterTable(code, source, dest, wrap, idx.ctypes.data, wgt.ctypes.data, cap)
                e = pins["tables"][name]
                assert n == e["entries"], (name, n)
                assert hashlib.sha256(_table_bytes(kind, idx[:n], wgt[:n])).hexdigest() == e["sha256"], name
                assert (idx[n:] == -7).all() and (wgt[n:] == -7.0).all()
    small = np.zeros((1, 2), dtype=np.int32)
    assert T.itwTestMipFilterTable(2, 12, 6, 0, small.ctypes.data, np.zeros(1, np.float32).ctypes.data, 1) == -1


def test_a_constant_image_stays_constant_under_cubic_exactly():
    for value in (0x3C00, 0xBC00, 0x7BFF, 0xFBFF, 0x0001, 0x0000):       # (every difference is 0 and a0 + 0 is a0; only -0 would become +0)
        base = np.full((20, 12, 4), value, dtype=np.uint16)
        for wrap in MF.WRAPS:
            assert all((lv == value).all() for lv in MF.chain(base, "cubic", wrap))
    for kind in ("rgba8", "srgb"):
        for code in (0, 1, 77, 254, 255):
            base = np.full((9, 33, 4), code, dtype=np.uint8)
            assert all((lv == code).all() for lv in MF.chain(base, "cubic", "uv", kind))


def test_cubic_at_the_2_to_1_ratio_is_the_four_tap_kernel():
    """x = 0.5 at 2:1: weights (-1, 9, 9, -1) / 16 per axis, here on codes small enough for every product and sum to be exact."""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 64, (16, 16, 4)).astype(np.float32)
    got = MF.cubic_unrounded(img, True, True)
    p = np.pad(img, ((1, 2), (1, 2), (0, 0)), mode="wrap").astype(np.float64)
    k = np.array([-1, 9, 9, -1]) / 16.0
    rows = sum(k[i] * p[:, i:i + 16:2][:, :8] for i in range(4))
    want = sum(k[i] * rows[i:i + 16:2][:8] for i in range(4))
    assert np.abs(got - want).max() < 1e-4                        # (third and sixth are rounded constants: not exact, but the kernel's shape)


def test_the_flag_constants_agree(itw):
    header = open(os.path.join(ROOT, "include", "itw_dispatch.h")).read()
    m = re.search(r"enum \{ ITW_MIP_PER_LEVEL = 1, ITW_MIP_SRGB = 4,\s*ITW_MIP_CUBIC = 0x10, ITW_MIP_TRIANGLE = 0x20, ITW_MIP_WRAP_U = 0x40, ITW_MIP_WRAP_V = 0x80 \};", header)
    assert m
    assert (itw.MIP_PER_LEVEL, itw.MIP_SRGB, itw.MIP_CUBIC, itw.MIP_TRIANGLE, itw.MIP_WRAP_U, itw.MIP_WRAP_V) == (1, 4, 0x10, 0x20, 0x40, 0x80)
    assert itw.mip_filter_flags() == 0 and itw.mip_filter_flags("cubic", "uv") == 0xD0 and itw.mip_filter_flags("triangle", "v") == 0xA0
    assert itw.mip_filter_flags(None, "u") == 0x40
    for bad in (("box", ""), ("cubic", "w"), ("cubic", "vu")):
        with pytest.raises(ValueError):
            itw.mip_filter_flags(*bad)


def test_the_product_library_lists_exactly_the_symbols_it_listed_before(itw):
    """The filters arrive through flag bits of the existing entry points: 132 exported functions, the same names."""
    out = subprocess.run(["nm", "-D", "--defined-only", itw.lib_path()], check=True, capture_output=True, text=True).stdout
    names = sorted(l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T")
    assert names == sorted(itw.EXPORTED_SYMBOLS) and len(names) == 132
    assert hashlib.sha256(("\n".join(names) + "\n").encode()).hexdigest() == "c95d9d1b784b2eba98e5209b41d4654268a44bb0ff28699e20a7fcae01dad85c"


def test_refusals_and_the_default_filter_in_a_fresh_interpreter():
    """Fresh interpreter: the error mode is process-wide.  Every refusal leaves a message, returns -1 / false and changes no byte; the
    wrap bits without a filter bit are accepted on a host chain and, where a GPU is present, give the bytes of flags 0."""
    code = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
import itw_amd
L = itw_amd.lib()
S = itw_amd.RgbaSurface
itw_amd.set_error_mode(itw_amd.ON_ERROR_RETURN)
store = np.full(8 * 8 * 8 * 2, 0x11, np.uint8)
p = store.ctypes.data
def chain(px=4, w=8, h=8):
    out = (S * 4)()
    assert L.itwMipChainLayout(w, h, 1, 4, px, p, C.cast(out, C.c_void_p)) > 0
    return out
def ptr(a):
    return C.cast(a, C.c_void_p)
def opts(*a, **k):
    o = itw_amd.MipAlpha(*a, **k)
    return o, C.cast(C.byref(o), C.c_void_p)
n = 0
def refused(what, call, word):
    global n
    L.itwClearError()
    assert call() in (-1, False), what
    assert word in itw_amd.last_error(), (what, itw_amd.last_error())
    n += 1
CU, TR, WU, WV = 0x10, 0x20, 0x40, 0x80
for px in (4, 8):
    for more in (0, 1, WU, WV | WU):
        refused("both filters", lambda: L.itwGenerateMipChain(ptr(chain(px)), 1, 4, px, CU | TR | more), "ITW_MIP_CUBIC and ITW_MIP_TRIANGLE")
    for bits in (2, 8, 0x80000000):
        for beside in (CU, TR, WU, WV, CU | WU | WV, 0x100):
            refused("bit 0x%%x beside 0x%%x" %% (bits, beside), lambda: L.itwGenerateMipChain(ptr(chain(px)), 1, 4, px, bits | beside), "unknown flag")
    refused("bit 0x100", lambda: L.itwGenerateMipChain(ptr(chain(px)), 1, 4, px, 0x100 | CU), "unknown flag")
refused("sRGB halves beside a filter", lambda: L.itwGenerateMipChain(ptr(chain(8)), 1, 4, 8, 4 | CU), "ITW_MIP_SRGB")
for f, name in ((CU, "ITW_MIP_CUBIC"), (TR, "ITW_MIP_TRIANGLE")):
    for cov in (0, 128):
        refused("weight_colour with " + name, lambda: L.itwGenerateMipChainAlpha(ptr(chain()), 1, 4, f | WU, opts(1, cov)[1], None), "weight_colour with " + name)
refused("both filters, alpha call", lambda: L.itwGenerateMipChainAlpha(ptr(chain()), 1, 4, CU | TR, opts(0, 128)[1], None), "ITW_MIP_CUBIC and ITW_MIP_TRIANGLE")
for bits in (2, 8, 0x80000000):
    refused("alpha call, bit 0x%%x" %% bits, lambda: L.itwGenerateMipChainAlpha(ptr(chain()), 1, 4, bits | TR, opts(0, 128)[1], None), "unknown flag")
bad = chain(); bad[2].width = 3
refused("a level of the wrong size under cubic", lambda: L.itwGenerateMipChain(ptr(bad), 1, 4, 4, CU), "level 2")
assert (store == 0x11).all()
print("generate refused", n)

out = np.full(4096, 0x33, np.uint8)
t = out.ctypes.data
img = np.zeros((8, 8, 4), np.uint8)
b8 = ptr((S * 1)(S(img.ctypes.data, 8, 8, 32)))
m = 0
def refused2(what, call, word):
    global m
    L.itwClearError()
    assert call() is False, what
    assert word in itw_amd.last_error(), (what, itw_amd.last_error())
    m += 1
refused2("both filters", lambda: L.itwCompressImageMippedEx(b8, 1, 0, 0, CU | TR, t, 71, None, None, None), "ITW_MIP_CUBIC and ITW_MIP_TRIANGLE")
refused2("both filters, alpha call", lambda: L.itwCompressImageMippedAlpha(b8, 1, 0, CU | TR | WV, opts(0, 128)[1], t, 77, None, None, None), "ITW_MIP_CUBIC and ITW_MIP_TRIANGLE")
for f, name in ((CU, "ITW_MIP_CUBIC"), (TR, "ITW_MIP_TRIANGLE")):
    refused2("weight_colour with " + name, lambda: L.itwCompressImageMippedAlpha(b8, 1, 0, f, opts(1, 0)[1], t, 77, None, None, None), "weight_colour with " + name)
for bits in (2, 8, 0x80000000):
    refused2("mip flag 0x%%x" %% bits, lambda: L.itwCompressImageMippedEx(b8, 1, 0, 0, bits | CU | WU, t, 71, None, None, None), "unknown mip flag")
    refused2("mip flag 0x%%x, alpha call" %% bits, lambda: L.itwCompressImageMippedAlpha(b8, 1, 0, bits | TR, opts(0, 128)[1], t, 77, None, None, None), "unknown mip flag")
refused2("sRGB with normal ops beside a filter", lambda: L.itwCompressImageMippedEx(b8, 1, 0, 4, 4 | CU, t, 71, None, None, None), "normal")
assert (out == 0x33).all()
print("mipped refused", m)

# the wrap bits alone: nothing to do returns 0 whatever the machine; with a GPU a host chain takes the bytes of flags 0
assert L.itwGenerateMipChain(ptr(chain()), 1, 1, 4, WU | WV) == 0 and L.itwGenerateMipChain(ptr(chain()), 0, 4, 4, WU) == 0
assert (store == 0x11).all()
if itw_amd.available():
    rng = np.random.default_rng(5)
    for shape, dtype in (((8, 8, 4), np.uint8), ((6, 5, 4), np.uint8), ((8, 8, 4), np.uint16), ((5, 12, 4), np.uint16)):
        base = rng.integers(0, 256 if dtype == np.uint8 else 0x7000, shape).astype(dtype)
        want = itw_amd.generate_mips(base)
        for wrap in ("u", "v", "uv"):
            got = itw_amd.generate_mips(base, wrap=wrap)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (shape, wrap)
    print("wrap alone: the bytes of flags 0")
else:
    L.itwClearError()
    assert L.itwGenerateMipChain(ptr(chain()), 1, 4, 4, WU | WV) == -1 and "unknown" not in itw_amd.last_error() and "ITW_MIP" not in itw_amd.last_error()
    print("wrap alone: accepted by the checks")
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.split("\n")
    assert lines[:2] == ["generate refused 56", "mipped refused 11"], lines
    assert lines[2] in ("wrap alone: the bytes of flags 0", "wrap alone: accepted by the checks")


def test_the_filter_kernels_have_no_scratch_and_no_spills():
    obj = os.path.join(CSRC, "build", "mip_filters.o")
    if not os.path.exists(obj):
        pytest.skip("csrc/build/ is not populated: run __graft_entry__.build() first")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), obj], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines():
        m = re.match(r"(?:void )?itw::(\S.*?)\s+vgpr\s+(\d+) agpr\s+(\d+) .*?scratch\s+(\d+) B\s+lds\s+(\d+) B\s+spills v(\d+) s(\d+)", line)
        if m:
            table[m.group(1)] = (int(m.group(2)) + int(m.group(3)), int(m.group(5)), int(m.group(4)), int(m.group(6)) + int(m.group(7)))
    kinds = ("<4, false>", "<4, true>", "<8, false>")
    assert set(table) == {k + t for k in ("mip_cubic_kernel", "mip_cubic_lds_kernel", "mip_triangle_kernel") for t in kinds}, sorted(table)
    for name, (regs, lds, scratch, spills) in table.items():
        assert scratch == 0 and spills == 0, (name, table[name])
        assert lds <= 16384 and regs <= 64, (name, table[name])          # eight waves a SIMD by registers, ten workgroups a CU by LDS
