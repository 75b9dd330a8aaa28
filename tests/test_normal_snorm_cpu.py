"""The signed normal-map path without a GPU (include/itw_dispatch.h, "signed normal sources"): the numpy model's round trips and tie rule
(tests/_normal_snorm.py), the refusals of itwQuantizeNormalMapChain, itwCompressNormalMapBC5S, itwCompressSignedNormalMapChain and
itwCompressSignedNormalMapMipped, which happen before any device work, and
the registers of the bc45_kernel instantiations read from the built code object."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _normal_snorm as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "intel-texture-works-plugin_amd", "csrc", "build", "bc4_bc5.o")
f32 = np.float32


def boundary_points():
    """fp32((k + 0.5) / 127) for k = -127 .. 126 with its three fp32 neighbours on either side: (254, 7)"""
    k = np.arange(-127, 127, dtype=np.float64)
    pts = [((k + 0.5) / 127.0).astype(f32)]
    lo = hi = pts[0]
    for _ in range(3):
        lo = np.nextafter(lo, f32(-2.0))
        hi = np.nextafter(hi, f32(2.0))
        pts += [lo, hi]
    return np.stack(pts, axis=1)


def test_all_codes_map_to_themselves_directly_and_through_a_half():
    codes = np.arange(-128, 128).astype(np.int8)
    want = np.where(codes == -128, -127, codes).astype(np.int8)
    img = np.repeat(codes[:, None], 4, axis=1)
    assert np.array_equal(S.quantize(img, 0), np.repeat(want[:, None], 4, axis=1))
    half = S.load(img).astype(np.float16)
    assert np.array_equal(S.quantize(half, 0), np.repeat(want[:, None], 4, axis=1))
    assert np.array_equal(S.quantize(half.view(np.uint16), 0), np.repeat(want[:, None], 4, axis=1))


def test_ties_round_to_even_and_minus_128_never_comes_out():
    pts = boundary_points()
    p = pts * f32(127.0)
    ties = (p.astype(np.float64) - np.floor(p.astype(np.float64))) == 0.5
    assert ties.sum() > 100                                       # exact k + 0.5 products occur: the tie rule decides codes
    q = S.quantize_values(pts).astype(np.int32)
    even = np.rint(p.astype(np.float64)).astype(np.int32)         # numpy rounds half to even
    away = (np.sign(p) * np.floor(np.abs(p.astype(np.float64)) + 0.5)).astype(np.int32)
    assert np.array_equal(q, even) and (q[ties] % 2 == 0).all()
    assert (even[ties] != away[ties]).any()                       # the points separate the two rules
    special = np.array([0.0, -0.0, 1.0, -1.0, 2.0, -2.0, np.inf, -np.inf, np.nan, 1e-45, np.nextafter(f32(1), f32(2)), np.nextafter(f32(-1), f32(-2))], dtype=f32)
    assert S.quantize_values(special).tolist() == [0, 0, 127, -127, 127, -127, 127, -127, 0, 0, 127, -127]
    everything = S.quantize_values(np.arange(65536, dtype=np.uint16).view(np.float16).astype(f32))
    assert everything.min() == -127 and everything.max() == 127


def test_the_normalise_defaults_and_flips():
    v = np.array([[0, 0, 0, 0.25], [np.nan, 0, 1, -3], [3, 4, 0, 0.5], [np.inf, 1, 1, 0]], dtype=f32)
    assert S.quantize(v, 4).tolist() == [[0, 0, 127, 32], [0, 0, 127, -127], [76, 102, 0, 64], [0, 0, 0, 0]]
    assert S.quantize(v[2:3], 7).tolist() == [[-76, -102, 0, 64]]
    assert S.quantize(v[2:3], 3).tolist() == [[-127, -127, 0, 64]]
    # the case the biased RGBA8 path gets wrong: int8 -1 and +1 average to 0, not to -128
    assert S.quantize(np.array([[-1, 1, 0, 0]], np.int8), 1).tolist() == [[1, 1, 0, 0]]


def test_bad_calls_are_refused_before_any_device_use():
    """Each bad call returns -1 (the void encoder: returns) with the refusal's own message under ITW_ON_ERROR_RETURN, on a box without a GPU
    as on one with it.  Run in a fresh interpreter: the error mode is process-wide."""
    code = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
import itw_amd
L = itw_amd.lib()
itw_amd.set_error_mode(itw_amd.ON_ERROR_RETURN)
S = itw_amd.RgbaSurface
src = np.zeros((8, 8, 4), dtype=np.float32)
dst = np.zeros((8, 8, 4), dtype=np.int8)
out = np.zeros(4096, dtype=np.uint8)
def arr(*s):
    return C.cast((S * len(s))(*s), C.c_void_p)
gs, gd = S(src.ctypes.data, 8, 8, 128), S(dst.ctypes.data, 8, 8, 32)
cases = {
    "null sources": (None, 16, arr(gd), 1, 0),
    "null targets": (arr(gs), 16, None, 1, 0),
    "null source texels": (arr(S(None, 8, 8, 128)), 16, arr(gd), 1, 0),
    "null target texels": (arr(gs), 16, arr(S(None, 8, 8, 32)), 1, 0),
    "count < 0": (arr(gs), 16, arr(gd), -1, 0),
    "texel_bytes 2": (arr(gs), 2, arr(gd), 1, 0),
    "texel_bytes 12": (arr(gs), 12, arr(gd), 1, 0),
    "ops 8": (arr(gs), 16, arr(gd), 1, 8),
    "width 0": (arr(S(src.ctypes.data, 0, 8, 128)), 16, arr(S(dst.ctypes.data, 0, 8, 32)), 1, 0),
    "height 0": (arr(S(src.ctypes.data, 8, 0, 128)), 16, arr(S(dst.ctypes.data, 8, 0, 32)), 1, 0),
    "target size": (arr(gs), 16, arr(S(dst.ctypes.data, 4, 8, 32)), 1, 0),
    "second image's target size": (arr(gs, gs), 16, arr(gd, S(dst.ctypes.data, 8, 4, 32)), 2, 0),
    "source stride": (arr(S(src.ctypes.data, 8, 8, 127)), 16, arr(gd), 1, 0),
    "target stride": (arr(gs), 16, arr(S(dst.ctypes.data, 8, 8, 31)), 1, 0),
    "source alignment": (arr(S(src.ctypes.data + 4, 4, 4, 128)), 16, arr(S(dst.ctypes.data, 4, 4, 32)), 1, 0),
    "half source alignment": (arr(S(src.ctypes.data + 4, 4, 4, 128)), 8, arr(S(dst.ctypes.data, 4, 4, 32)), 1, 0),
    "source stride alignment": (arr(S(src.ctypes.data, 4, 4, 132)), 16, arr(S(dst.ctypes.data, 4, 4, 32)), 1, 0),
    "target alignment": (arr(gs), 16, arr(S(dst.ctypes.data + 2, 8, 8, 32)), 1, 0),
}
for name, (s, tb, t, n, ops) in cases.items():
    L.itwClearError()
    r = L.itwQuantizeNormalMapChain(s, tb, t, n, ops)
    err = itw_amd.last_error()
    assert r == -1 and err and "itwQuantizeNormalMapChain" in err, (name, r, err)
L.itwClearError()
assert L.itwQuantizeNormalMapChain(None, 16, None, 0, 7) == 0 and not itw_amd.last_error()       # count 0: nothing to do
enc = {
    "texel_bytes 2": (C.byref(gs), 2, out.ctypes.data, 0, "texel_bytes"),
    "texel_bytes 0": (C.byref(gs), 0, out.ctypes.data, 7, "texel_bytes"),
    "ops 8": (C.byref(gs), 16, out.ctypes.data, 8, "ops"),
    "ops 8, int8": (C.byref(gd), 4, out.ctypes.data, 8, "ops"),
    "null surface": (None, 16, out.ctypes.data, 7, "null"),
    "null texels": (C.byref(S(None, 8, 8, 128)), 16, out.ctypes.data, 7, "null"),
    "null dst": (C.byref(gs), 16, None, 7, "null"),
}
for name, (s, tb, d, ops, word) in enc.items():
    L.itwClearError()
    out[:] = 0xA5
    L.itwCompressNormalMapBC5S(s, tb, d, ops)
    err = itw_amd.last_error()
    assert err and word in err and "hip" not in err.lower(), (name, err)
    assert (out == 0xA5).all(), name
chain = {
    "format 83 (BC5_UNORM)": (arr(gs), 1, 16, out.ctypes.data, 83, 0),
    "format 98 (BC7)": (arr(gs), 1, 16, out.ctypes.data, 98, 0),
    "format 0": (arr(gs), 1, 16, out.ctypes.data, 0, 0),
    "texel_bytes 2": (arr(gs), 1, 2, out.ctypes.data, 84, 0),
    "ops 8": (arr(gs), 1, 16, out.ctypes.data, 84, 8),
    "count 0": (arr(gs), 0, 16, out.ctypes.data, 84, 0),
    "null images": (None, 1, 16, out.ctypes.data, 81, 0),
    "null target": (arr(gs), 1, 16, None, 84, 0),
    "null texels": (arr(S(None, 8, 8, 128)), 1, 16, out.ctypes.data, 84, 0),
    "0-width image": (arr(gs, S(src.ctypes.data, 0, 8, 128)), 2, 16, out.ctypes.data, 81, 0),
    "stride below the float row": (arr(S(src.ctypes.data, 8, 8, 64)), 1, 16, out.ctypes.data, 84, 0),
    "stride below the half row": (arr(S(src.ctypes.data, 8, 8, 32)), 1, 8, out.ctypes.data, 84, 0),
}
for name, (images, count, tb, target, fmt, ops) in chain.items():
    L.itwClearError()
    out[:] = 0xA5
    ok = L.itwCompressSignedNormalMapChain(images, count, tb, target, fmt, ops, None, None)
    err = itw_amd.last_error()
    assert ok is False and err and "hip" not in err.lower(), (name, ok, err)
    assert (out == 0xA5).all(), name
f32b = S(src.ctypes.data, 8, 8, 128)
mipped = {
    "format 83": (arr(f32b), 1, 0, 16, 0, out.ctypes.data, 83),
    "texel_bytes 3": (arr(f32b), 1, 0, 3, 0, out.ctypes.data, 84),
    "ops 16": (arr(f32b), 1, 0, 16, 16, out.ctypes.data, 84),
    "items 0": (arr(f32b), 0, 0, 16, 0, out.ctypes.data, 84),
    "null bases": (None, 1, 0, 16, 0, out.ctypes.data, 84),
    "null target": (arr(f32b), 1, 0, 16, 0, None, 84),
    "null texels": (arr(S(None, 8, 8, 128)), 1, 0, 16, 0, out.ctypes.data, 84),
    "bases of two sizes": (arr(f32b, S(src.ctypes.data, 4, 4, 128)), 2, 0, 16, 0, out.ctypes.data, 84),
    "stride below the row": (arr(S(src.ctypes.data, 8, 8, 64)), 1, 0, 16, 0, out.ctypes.data, 84),
    "texels not aligned": (arr(S(src.ctypes.data + 4, 4, 4, 128)), 1, 0, 16, 0, out.ctypes.data, 81),
    "5 levels of an 8 x 8 base": (arr(f32b), 1, 5, 16, 0, out.ctypes.data, 84),
    "levels < 0": (arr(f32b), 1, -1, 16, 0, out.ctypes.data, 84),
}
for name, (bases, items, levels, tb, ops, target, fmt) in mipped.items():
    L.itwClearError()
    out[:] = 0xA5
    ok = L.itwCompressSignedNormalMapMipped(bases, items, levels, tb, ops, target, fmt, None, None)
    err = itw_amd.last_error()
    assert ok is False and err and "hip" not in err.lower(), (name, ok, err)
    assert (out == 0xA5).all(), name
print("refused", len(cases), len(enc), len(chain), len(mipped))
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "refused 18 7 12 12"


# ---- the code object -----------------------------------------------------------------------------------------------------------------
# bc45_kernel<NCH, VEC16, WHOLE, SGN, PREP>: VGPRs of every instantiation on the parent commit, read from its build with the same compiler.
# PREP 1..7 are itwCompressNormalMapBC5's, identical per (VEC16, WHOLE).
PARENT_VGPRS = {("1", v, w, "false", "0u"): 128 for v in ("false", "true") for w in ("false", "true")}
PARENT_VGPRS.update({("1", v, w, "true", "0u"): 127 for v in ("false", "true") for w in ("false", "true")})
PARENT_VGPRS.update({("2", v, w, s, "0u"): 128 for v in ("false", "true") for w in ("false", "true") for s in ("false", "true")})
PARENT_VGPRS.update({("2", v, w, "false", f"{p}u"): 128 for v in ("false", "true") for w in ("false", "true") for p in range(1, 8)})
# what itwCompressNormalMapBC5S launches: PREP = 16 * texel_bytes, and waves per SIMD each holds: a whole-block float
# surface keeps 24 prefetched words in flight and is budgeted for three waves, everything else for four
NEW_WAVES = {("2", v, w, "true", p): (3 if (p == "256u" and w == "true") else 4) for v in ("false", "true") for w in ("false", "true") for p in ("64u", "128u", "256u")}


def _bc45_table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as K
    with tempfile.TemporaryDirectory() as d:
        notes = K.kernel_notes(K.unbundle(OBJ, d))
    table = {}
    for k in notes:
        name = K.note_field(k, "name")
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        i = dem.find("bc45_kernel<")
        if i < 0:
            continue
        args = tuple(a.strip() for a in dem[i + len("bc45_kernel<"):dem.index(">", i)].split(","))
        table[args] = {f: int(K.note_field(k, f)) for f in ("vgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    return table


@pytest.fixture(scope="module")
def bc45_table():
    if not os.path.exists(OBJ):
        pytest.skip("csrc/build/ is not populated: run __graft_entry__.build() first")
    return _bc45_table()


def test_the_signed_normal_instantiations_have_no_scratch_and_hold_their_waves(bc45_table):
    for args, want in NEW_WAVES.items():
        assert args in bc45_table, (args, sorted(bc45_table))
        r = bc45_table[args]
        assert r["private_segment_fixed_size"] == 0, (args, r)
        regs = r["vgpr_count"] + r["agpr_count"]
        by_regs = 512 // (-(-regs // 8) * 8)
        by_lds = (160 * 1024) // r["group_segment_fixed_size"] if r["group_segment_fixed_size"] else 8
        assert min(by_regs, by_lds, 8) == want, (args, r)


def test_the_earlier_instantiations_keep_their_registers(bc45_table):
    assert set(bc45_table) == set(PARENT_VGPRS) | set(NEW_WAVES)
    for args, want in PARENT_VGPRS.items():
        r = bc45_table[args]
        assert r["vgpr_count"] == want and r["agpr_count"] == 0 and r["private_segment_fixed_size"] == 0, (args, r, want)
