"""The mip rules for cut-out textures without a GPU (include/itw_dispatch.h, "Mip chains of cut-out textures"): the model of
tests/_alpha_mips.py against itself (the fp32 and the integer form of the weighted box, the consequences of the coverage rule), every
refusal of the three calls before any device work, the structs' sizes, and the scratch and spills of csrc/build/mip_alpha.o."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _alpha_mips as A
import _mipgen as M
import _srgb_mips as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "intel-texture-works-plugin_amd", "csrc")


def test_the_models_filters_are_the_plain_models():
    """box_filter / linear_filter restate tests/_mipgen.py's expressions: stored, they are its levels; and with every alpha 255 the weighted
    level is the plain one wherever the division is exact -- on constant colour."""
    rng = np.random.default_rng(1)
    for h, w in ((8, 16), (1, 8), (8, 1), (2, 2)):
        img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        assert np.array_equal(M.store(A.box_filter(M.widen(img)), np.uint8), M.box_level(img))
    for h, w in ((5, 3), (19, 37), (7, 1)):
        img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        assert np.array_equal(M.store(A.linear_filter(M.widen(img)), np.uint8), M.linear_level(img))
        assert np.array_equal(S.store(A.linear_filter(S.widen(img)), np.uint8), S.linear_level(img))
    flat = np.full((8, 8, 4), 200, np.uint8)
    for srgb in (False, True):
        assert all((lv == 200).all() for lv in A.chain(flat, weight=True, srgb=srgb)[0])


def test_the_fp32_and_integer_forms_of_the_weighted_box_agree_on_every_pair():
    """den = sum(a) = 1 .. 1020, num = sum(a c) = 0 .. 255 * den: 132 782 070 pairs."""
    pairs = 0
    for den in range(1, 1021):
        num = np.arange(0, 255 * den + 1, dtype=np.int64)
        d = np.full(num.shape, den, dtype=np.int64)
        assert np.array_equal(A.weighted_ratio_fp32(num, d), A.weighted_ratio_integer(num, d)), den
        pairs += num.size
    assert pairs == 132782070


def test_the_integer_box_is_the_fp32_box_on_images():
    for seed, (h, w) in enumerate(((16, 16), (1, 8), (8, 1), (2, 2), (32, 8))):
        for img in (A.cutout(h, w, seed), A.noise(h, w, seed)):
            assert np.array_equal(A.weighted_level(img), A.box_level_weighted_integer(img))
    # invisible colour stays out: a visible red texel beside three transparent green ones
    img = np.array([[[255, 0, 0, 255], [0, 255, 0, 0]], [[0, 255, 0, 0], [0, 255, 0, 0]]], dtype=np.uint8)
    assert A.weighted_level(img)[0, 0].tolist() == [255, 0, 0, 64] and M.box_level(img)[0, 0].tolist() == [64, 191, 0, 64]
    img[..., 3] = 0                                                # nothing visible: the plain rule's colour
    assert A.weighted_level(img)[0, 0].tolist() == M.box_level(img)[0, 0].tolist() == [64, 191, 0, 0]


def _random_hist(rng, kind):
    if kind == 0:
        return rng.integers(0, 50, 256)
    if kind == 1:                                                  # two spikes and a little between
        h = rng.integers(0, 3, 256)
        h[0], h[255] = rng.integers(100, 5000, 2)
        return h
    h = np.zeros(256, dtype=np.int64)                              # a few occupied bins
    h[rng.integers(0, 256, rng.integers(1, 5))] = rng.integers(1, 1000)
    return h


def test_the_consequences_of_the_coverage_rule():
    rng = np.random.default_rng(7)
    codes = np.arange(256)
    for trial in range(600):
        hist = _random_hist(rng, trial % 3).astype(np.int64)
        n, r = int(hist.sum()), int(rng.integers(1, 256))
        k = int(rng.integers(0, n + 1))
        t = A.threshold(hist, k, r)
        ge = A.ge_counts(hist)
        lut = A.rescale(codes, r, t)
        assert 1 <= t <= 255
        assert int(hist[lut >= r].sum()) == ge[t]                  # #(a' >= r) == ge[t*]: a < t*  =>  a r / t* < r
        assert lut[0] == 0 and (np.diff(lut.astype(int)) >= 0).all()
        if t == r:
            assert np.array_equal(lut, codes)                      # identity
        # the third key never decides: ge is non-increasing, so of r - d and r + d with equal misses r itself misses no more and is nearer
        best = min(abs(ge[u] - k) for u in range(1, 256))
        nearest = min(abs(u - r) for u in range(1, 256) if abs(ge[u] - k) == best)
        assert [u for u in range(1, 256) if abs(ge[u] - k) == best and abs(u - r) == nearest] == [t]


def test_the_order_of_the_tie_breaks():
    hist = np.zeros(256, dtype=np.int64)
    hist[0], hist[255] = 10, 6                                     # ge[t] = 6 for every t in 1 .. 255: all miss alike, the nearest to r wins
    for r in (1, 128, 255):
        assert A.threshold(hist, 3, r) == r
    hist = np.zeros(256, dtype=np.int64)
    hist[100], hist[200] = 5, 5                                    # ge: 10 up to 100, 5 up to 200, 0 above
    assert A.threshold(hist, 5, 128) == 128                        # the miss first: the whole middle plateau hits K, r is in it
    assert A.threshold(hist, 10, 128) == 100                       # the plateau 1 .. 100 hits K; 100 is its nearest to r
    assert A.threshold(hist, 0, 128) == 201
    assert A.threshold(hist, 7, 150) == 150                        # misses 3 (t <= 100), 2 (101 .. 200), 7: the middle plateau, r in it
    assert A.threshold(hist, 8, 150) == 100                        # misses 2, 3, 8: the first plateau although r is not in it, its nearest to r
    assert A.threshold(hist, 8, 30) == 30 and A.threshold(hist, 2, 250) == 250


def test_the_target_at_the_ends():
    for n0, n in ((4096, 1024), (130 * 66, 65 * 33), (7, 3), (1 << 31, 1 << 29)):
        assert A.target(0, n, n0) == 0
        assert A.target(n0, n, n0) == n
        assert A.target(n0 // 2, n, n0) in (n // 2, n // 2 + 1, (n + 1) // 2)
    assert A.target(5, 1, 8) == 1 and A.target(3, 1, 8) == 0 and A.target(4, 1, 8) == 1     # round half up on a 1 x 1 level


def test_the_chain_applies_coverage_after_the_whole_chain():
    base = A.cutout(32, 32, 3, hole=False)
    plain, none = A.chain(base, weight=True)
    kept, rows = A.chain(base, weight=True, ref=128)
    assert none is None and len(rows) == len(kept) == 6
    a0 = base[..., 3]
    assert rows[0] == (1024, int((a0 >= 128).sum()), int((a0 >= 128).sum()), 128)
    for lv, pl, row in zip(kept[1:], plain[1:], rows[1:]):
        assert np.array_equal(lv[..., :3], pl[..., :3])            # R, G, B never touched
        assert row[0] == lv[..., 3].size and row[1] == int((pl[..., 3] >= 128).sum()) and row[2] == int((lv[..., 3] >= 128).sum())
        assert ((pl[..., 3] == 0) <= (lv[..., 3] == 0)).all()      # alpha 0 stays 0


def test_struct_sizes_and_symbols(itw):
    assert C.sizeof(itw.MipAlpha) == 16 and C.sizeof(itw.MipCoverage) == 32
    L = itw.lib()
    for name in ("itwGenerateMipChainAlpha", "itwCompressImageMippedAlpha", "itwAlphaCoverage"):
        assert name in itw.EXPORTED_SYMBOLS and hasattr(L, name)
    header = open(os.path.join(ROOT, "include", "itw_dispatch.h")).read()
    assert "uint32_t struct_size /* 16 */, weight_colour /* 0|1 */, coverage_ref /* 0..255 */, reserved /* 0 */; } itw_mip_alpha;" in header
    assert "uint64_t texels, covered_plain, covered; uint32_t threshold, reserved; } itw_mip_coverage;" in header


def test_noops_return_zero_and_write_nothing(itw):
    L = itw.lib()
    img = np.full((8, 8, 4), 0xA5, np.uint8)
    arr = C.cast((itw.RgbaSurface * 1)(itw.RgbaSurface(img.ctypes.data, 8, 8, 32)), C.c_void_p)
    opts = itw.MipAlpha(1, 128)
    assert L.itwGenerateMipChainAlpha(arr, 0, 2, 0, C.cast(C.byref(opts), C.c_void_p), None) == 0
    assert L.itwGenerateMipChainAlpha(arr, 1, 1, 5, C.cast(C.byref(opts), C.c_void_p), None) == 0
    assert L.itwGenerateMipChainAlpha(arr, 1, 1, 0, None, None) == 0
    assert L.itwAlphaCoverage(arr, 0, 128, None) == 0
    assert (img == 0xA5).all()


def test_refusals_come_before_any_device_use():
    """Fresh interpreter: the error mode is process-wide.  Every refusal leaves a message, returns -1 / false and changes no byte."""
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
rows = (itw_amd.MipCoverage * 4)()
C.memset(rows, 0x22, C.sizeof(rows))
n = 0
def refused(what, images, flags, o, report, word):
    global n
    L.itwClearError()
    assert L.itwGenerateMipChainAlpha(ptr(images) if images is not None else None, 1, 4, flags, o[1] if o else None, ptr(report) if report is not None else None) == -1, what
    assert word in itw_amd.last_error(), (what, itw_amd.last_error())
    n += 1
refused("struct_size 12", chain(), 0, opts(1, 128, struct_size=12), None, "struct_size")
refused("struct_size 0", chain(), 0, opts(0, 0, struct_size=0), None, "struct_size")
refused("reserved", chain(), 0, opts(1, 128, reserved=1), None, "reserved")
refused("weight_colour 2", chain(), 0, opts(2, 0), None, "weight_colour")
refused("coverage_ref 256", chain(), 0, opts(0, 256), None, "coverage_ref")
refused("a report without coverage", chain(), 0, opts(1, 0), rows, "report")
refused("a report without options", chain(), 0, None, rows, "report")
for bits in (2, 8, 0x80000000, 6, 1 | 8):
    refused("flag bits 0x%%x" %% bits, chain(), bits, opts(1, 128), None, "unknown flag")
    refused("flag bits 0x%%x, options off" %% bits, chain(), bits, None, None, "unknown flag")
refused("null images", None, 0, opts(1, 128), None, "null images")
bad = chain(); bad[2].width = 3
refused("a level of the wrong size", bad, 0, opts(1, 128), rows, "level 2")
bad = chain(); bad[1].ptr = None
refused("a null level", bad, 4, opts(0, 1), None, "null texel pointer")
bad = chain(); bad[1].stride = 8
refused("a short stride", bad, 0, opts(1, 0), None, "stride")
bad = chain(); bad[1].ptr = bad[1].ptr + 2
refused("misaligned texels", bad, 0, opts(1, 0), None, "aligned")
L.itwClearError()
assert L.itwGenerateMipChainAlpha(ptr(chain()), -1, 4, 0, opts(1, 1)[1], None) == -1 and "items" in itw_amd.last_error()
L.itwClearError()
assert L.itwGenerateMipChainAlpha(ptr(chain()), 1, 5, 0, opts(1, 1)[1], None) == -1 and "levels" in itw_amd.last_error()
assert (store == 0x11).all() and bytes(rows) == b"\x22" * C.sizeof(rows)
print("generate refused", n)

out = np.full(4096, 0x33, np.uint8)
t = out.ctypes.data
img = np.zeros((8, 8, 4), np.uint8)
half = np.zeros((8, 8, 4), np.uint16)
b8 = ptr((S * 1)(S(img.ctypes.data, 8, 8, 32)))
b16 = ptr((S * 1)(S(half.ctypes.data, 8, 8, 64)))
bc7 = itw_amd.bc7_profile("ultrafast")
s7 = C.cast(C.byref(bc7), C.c_void_p)
bc6 = itw_amd.bc6h_profile("veryfast")
s6 = C.cast(C.byref(bc6), C.c_void_p)
m = 0
def refused2(what, bases, flags, o, fmt, settings, word, target=t):
    global m
    L.itwClearError()
    assert L.itwCompressImageMippedAlpha(bases, 1, 0, flags, o[1] if o else None, target, fmt, settings, None, None) is False, what
    assert word in itw_amd.last_error(), (what, itw_amd.last_error())
    m += 1
for fmt, bases, settings in ((95, b16, s6), (96, b16, s6), (81, b8, None), (84, b8, None)):
    refused2("format %%d" %% fmt, bases, 0, opts(1, 128), fmt, settings, "DXGI format %%d" %% fmt)
    refused2("format %%d, options off" %% fmt, bases, 0, None, fmt, settings, "DXGI format %%d" %% fmt)
refused2("struct_size", b8, 0, opts(1, 128, struct_size=20), 77, None, "struct_size")
refused2("reserved", b8, 0, opts(1, 128, reserved=7), 77, None, "reserved")
refused2("weight_colour", b8, 0, opts(3, 128), 98, s7, "weight_colour")
refused2("coverage_ref", b8, 0, opts(1, 1000), 98, s7, "coverage_ref")
for bits in (2, 8, 0x80000000):
    refused2("mip flag bits 0x%%x" %% bits, b8, bits, opts(1, 128), 77, None, "unknown mip flag")
refused2("null BC7 settings", b8, 0, opts(1, 128), 98, None, "settings")
refused2("null target", b8, 0, opts(1, 128), 77, None, "", target=None)
assert (out == 0x33).all()
print("mipped refused", m)

cov = (C.c_uint64 * 2)(0x4444, 0x4444)
k = 0
def refused3(what, images, count, ref, covered, word):
    global k
    L.itwClearError()
    assert L.itwAlphaCoverage(images, count, ref, covered) == -1, what
    assert word in itw_amd.last_error(), (what, itw_amd.last_error())
    k += 1
refused3("ref 256", b8, 1, 256, ptr(cov), "alpha_ref")
refused3("ref -1", b8, 1, -1, ptr(cov), "alpha_ref")
refused3("count -1", b8, -1, 128, ptr(cov), "images")
refused3("null images", None, 1, 128, ptr(cov), "null images")
refused3("null covered", b8, 1, 128, None, "null covered")
refused3("a null texel pointer", ptr((S * 1)(S(None, 8, 8, 32))), 1, 128, ptr(cov), "null texel pointer")
refused3("an empty image", ptr((S * 1)(S(img.ctypes.data, 0, 8, 32))), 1, 128, ptr(cov), "0 x 8")
refused3("a short stride", ptr((S * 1)(S(img.ctypes.data, 8, 8, 16))), 1, 128, ptr(cov), "stride")
refused3("misaligned texels", ptr((S * 1)(S(img.ctypes.data + 1, 4, 4, 32))), 1, 128, ptr(cov), "aligned")
assert list(cov) == [0x4444, 0x4444]
print("coverage refused", k)
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.split("\n")[:3] == ["generate refused 22", "mipped refused 17", "coverage refused 9"]


def test_the_alpha_kernels_have_no_scratch_and_no_spills():
    obj = os.path.join(CSRC, "build", "mip_alpha.o")
    if not os.path.exists(obj):
        pytest.skip("csrc/build/ is not populated: run __graft_entry__.build() first")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), obj], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines():
        m = re.match(r"(?:void )?itw::(\S.*?)\s+vgpr\s+(\d+) agpr\s+(\d+) .*?scratch\s+(\d+) B\s+lds\s+(\d+) B\s+spills v(\d+) s(\d+)", line)
        if m:
            table[m.group(1)] = (int(m.group(2)) + int(m.group(3)), int(m.group(5)), int(m.group(4)), int(m.group(6)) + int(m.group(7)))
    assert set(table) == {"mip_alpha_pyramid_kernel<false>", "mip_alpha_pyramid_kernel<true>", "mip_alpha_tail_kernel<false>", "mip_alpha_tail_kernel<true>",
                          "mip_alpha_level_kernel<false, false>", "mip_alpha_level_kernel<true, false>", "mip_alpha_level_kernel<false, true>",
                          "mip_alpha_level_kernel<true, true>", "mip_alpha_hist_kernel<true>", "mip_alpha_hist_kernel<false>", "mip_alpha_select_kernel",
                          "mip_alpha_rescale_kernel"}, sorted(table)
    for name, (regs, lds, scratch, spills) in table.items():
        assert scratch == 0 and spills == 0, (name, table[name])
        assert lds <= 8192 and regs <= 128, (name, table[name])          # four workgroups a CU and more under both limits
