"""The sRGB colour kind of the mip filters without a GPU (include/itw_dispatch.h, "Mip chains", ITW_MIP_SRGB): csrc/srgb_tables.h and the
two host functions against the `decimal` model of tests/_srgb_mips.py, the facts the definition was chosen for, every refusal that must come
before device work, and the registers / LDS / scratch of the mip kernels' code objects."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _mipgen as M
import _srgb_mips as S

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "intel-texture-works-plugin_amd", "csrc")


def _header_table(name):
    src = open(os.path.join(CSRC, "srgb_tables.h")).read()
    body = re.search(r"constexpr uint32_t " + name + r"\[256\] = \{(.*?)\};", src, re.S).group(1)
    words = [int(x, 16) for x in re.findall(r"0x([0-9a-f]{8})u", body)]
    assert len(words) == 256
    return np.array(words, dtype=np.uint32).view(F)


def test_the_header_holds_the_decimal_models_tables():
    dec, thr = _header_table("SRGB_DECODE_BITS"), _header_table("SRGB_THR_BITS")
    assert np.array_equal(dec.view(np.uint32), S.DECODE.view(np.uint32))                       # 256 values
    assert np.array_equal(thr[1:].view(np.uint32), S.THR[1:].view(np.uint32)) and thr.view(np.uint32)[0] == 0      # 255 values
    assert dec[0] == 0.0 and dec[255] == 1.0


def test_the_generator_reproduces_the_committed_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_srgb_tables.py"), "--check"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


def test_the_tables_are_strictly_increasing_and_interleave():
    assert (np.diff(S.THR[1:]) > 0).all() and (np.diff(S.DECODE) > 0).all()
    assert S.THR[1] > 0
    assert (S.THR[1:] < S.DECODE[1:]).all() and (S.DECODE[:-1] < S.THR[1:]).all()             # T[c] < D[c] < T[c + 1]
    assert np.array_equal(S.encode(S.DECODE), np.arange(256, dtype=np.uint8))


def test_the_host_functions_are_the_definition(itw):
    L = itw.lib()
    assert [L.itwSrgbToLinear(c) for c in range(256)] == [float(v) for v in S.DECODE]
    assert [itw.srgb_to_linear(c) for c in (0, 1, 128, 255)] == [float(S.DECODE[c]) for c in (0, 1, 128, 255)]
    values = np.concatenate([S.threshold_neighbourhood(), np.random.default_rng(5).random(4096, dtype=F), np.array([2.0, 1e30, np.inf, -1.0], dtype=F)])
    want = S.encode(values)
    assert np.array_equal(want, S.encode_by_counting(values))                                  # searchsorted is the counting definition
    got = np.array([L.itwLinearToSrgb(float(v)) for v in values], dtype=np.uint8)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    for k in range(1, 256):                                                                    # a value equal to a threshold goes up
        assert itw.linear_to_srgb(S.THR[k]) == k and itw.linear_to_srgb(np.nextafter(S.THR[k], F(0))) == k - 1
    assert [itw.linear_to_srgb(v) for v in (0.0, -0.0, 1e-45, 1.0, float(np.nextafter(F(1), F(2))), 1.5, float("nan"))] == [0, 0, 0, 255, 255, 255, 0]


def _box(a, b, c, d):
    img = np.array([[[a] * 4, [c] * 4], [[b] * 4, [d] * 4]], dtype=np.uint8)                   # p0 p2 / p1 p3 (tests/_mipgen.py box_level)
    return S.box_level(img)[0, 0]


def test_the_facts_the_definition_was_chosen_for():
    plain = lambda *q: int(M.box_level(np.array(q, dtype=np.uint8).reshape(2, 2, 1).repeat(4, axis=2))[0, 0, 0])
    assert _box(0, 255, 0, 255).tolist() == [188, 188, 188, 128] and plain(0, 0, 255, 255) == 128
    assert _box(0, 0, 0, 255).tolist() == [137, 137, 137, 64]
    assert _box(64, 128, 192, 255).tolist() == [179, 179, 179, 160]
    assert _box(0, 1, 0, 1).tolist()[:3] == [1, 1, 1]                                         # exactly T[1]: goes up
    x = S.DECODE[1]
    assert F(F(F(F(0) + x) + F(0)) + x) * F(0.25) == S.THR[1]
    # every constant keeps its code: ((x + x) + x) + x) * 0.25f of D[c] encodes to c, far from any threshold
    x = S.DECODE
    v = (((x + x) + x) + x) * F(0.25)
    assert v.dtype == F and np.array_equal(S.encode(v), np.arange(256, dtype=np.uint8))
    bits = v.view(np.uint32).astype(np.int64)
    tb = S.THR[1:].view(np.uint32).astype(np.int64)
    gap = np.abs(bits[:, None] - tb[None, :]).min(axis=1)
    assert gap.min() > 37000, int(gap.min())                                                   # ulps to the nearest threshold
    for c in range(256):
        base = np.full((8, 8, 4), c, dtype=np.uint8)
        assert all((lv == c).all() for lv in S.chain(base)), c
    lin = np.full((5, 3, 4), 200, dtype=np.uint8)                                              # and under the linear filter
    assert all((lv == 200).all() for lv in S.chain(lin))


def test_the_model_is_the_plain_models_filters_around_other_ends():
    """Alpha follows the plain rule texel for texel, and a chain's colour differs from the plain chain's (the flag is not a no-op)."""
    img = np.random.default_rng(9).integers(0, 256, (16, 8, 4), dtype=np.uint8)
    a, b = S.chain(img), M.chain(img)
    assert all(np.array_equal(x[..., 3], y[..., 3]) for x, y in zip(a, b))
    assert any(not np.array_equal(x[..., :3], y[..., :3]) for x, y in zip(a, b))
    assert M.widen is not S.widen and M.store is not S.store                                   # the swap was undone


def test_the_devices_guess_stays_within_one_code_with_room_to_spare():
    """csrc/mipgen.hpp mip_srgb_encode corrects a guess by one compare either side, which is the definition whenever |guess - E| <= 1.  The
    guess restated with the host's log2 / exp2 and an error of +-0.05 codes added -- fifty times what two 1-ulp instructions and the fp32
    operations around them can give -- on every float within 4096 ulps of every threshold, the edge values and 2^20 seeded floats."""
    bits = S.THR[1:].view(np.uint32).astype(np.int64)
    near = (bits[:, None] + np.arange(-4096, 4097)[None, :]).reshape(-1).astype(np.uint32).view(F)
    v = np.concatenate([near, S.threshold_neighbourhood(), np.random.default_rng(3).random(1 << 20, dtype=F), np.array([2.0, 1e30], dtype=F)])
    with np.errstate(divide="ignore"):
        power = (F(269.025) * np.exp2((np.log2(v).astype(F) * F(1.0 / 2.4)).astype(F)).astype(F)).astype(F) - F(14.025)
    c = np.where(v > F(0.0031308), power, (v * F(12.92 * 255.0)).astype(F)).astype(F)
    want = S.encode(v).astype(np.int64)
    for err in (-0.05, 0.0, 0.05):
        g = np.minimum(np.maximum((c + F(err)) + F(0.5), F(0)), F(255)).astype(np.int64)
        assert np.abs(g - want).max() <= 1, err
        thr = np.concatenate([[F(np.nan)], S.THR[1:], [F(np.nan)]]).astype(F)                  # T[0] and T[256]: NaN, neither end moves
        with np.errstate(invalid="ignore"):
            fixed = g - (v < thr[g]) + (v >= thr[g + 1])
        assert np.array_equal(fixed, want), err


def test_flag_noops_return_zero(itw):
    """items == 0 and levels <= 1 with ITW_MIP_SRGB: nothing to do, and the flag is a known one (alone and with ITW_MIP_PER_LEVEL)."""
    L = itw.lib()
    assert itw.MIP_SRGB == 4 and itw.MIP_PER_LEVEL == 1
    img = np.full((8, 8, 4), 0xA5, np.uint8)
    arr = C.cast((itw.RgbaSurface * 1)(itw.RgbaSurface(img.ctypes.data, 8, 8, 32)), C.c_void_p)
    assert L.itwGenerateMipChain(arr, 0, 2, 4, 4) == 0
    assert L.itwGenerateMipChain(arr, 1, 1, 4, 5) == 0
    assert (img == 0xA5).all()


def test_refusals_come_before_any_device_use():
    """Fresh interpreter: the error mode is process-wide.  Every refusal leaves a message that names its reason and writes nothing."""
    code = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
import itw_amd
L = itw_amd.lib()
S = itw_amd.RgbaSurface
itw_amd.set_error_mode(itw_amd.ON_ERROR_RETURN)
store = np.full(8 * 8 * 8 * 2, 0x11, np.uint8)
p = store.ctypes.data
def chain(px):
    out = (S * 4)()
    assert L.itwMipChainLayout(8, 8, 1, 4, px, p, C.cast(out, C.c_void_p)) > 0
    return C.cast(out, C.c_void_p)
n = 0
def refused(what, images, px, flags, word):
    global n
    L.itwClearError()
    assert L.itwGenerateMipChain(images, 1, 4, px, flags) == -1, what
    assert word in itw_amd.last_error(), (what, itw_amd.last_error())
    n += 1
refused("sRGB with RGBA16F", chain(8), 8, 4, "ITW_MIP_SRGB")
refused("sRGB per level with RGBA16F", chain(8), 8, 5, "ITW_MIP_SRGB")
refused("sRGB with RGBA16F, no images", None, 8, 4, "ITW_MIP_SRGB")
refused("bit 2 stays unassigned", chain(4), 4, 2, "unknown flag")
refused("bit 2 beside the flag", chain(4), 4, 6, "unknown flag")
refused("bit 8", chain(4), 4, 12, "unknown flag")
print("generate refused", n)

out = np.zeros(4096, np.uint8)
t = out.ctypes.data
img = np.zeros((8, 8, 4), np.uint8)
half = np.zeros((8, 8, 4), np.uint16)
b8 = C.cast((S * 1)(S(img.ctypes.data, 8, 8, 32)), C.c_void_p)
b16 = C.cast((S * 1)(S(half.ctypes.data, 8, 8, 64)), C.c_void_p)
bc7 = itw_amd.bc7_profile("ultrafast")
s7 = C.cast(C.byref(bc7), C.c_void_p)
bc6 = itw_amd.bc6h_profile("veryfast")
s6 = C.cast(C.byref(bc6), C.c_void_p)
m = 0
def refused2(what, bases, ops, flags, fmt, settings, word):
    global m
    L.itwClearError()
    assert L.itwCompressImageMippedEx(bases, 1, 0, ops, flags, t, fmt, settings, None, None) is False, what
    assert word in itw_amd.last_error(), (what, itw_amd.last_error())
    m += 1
refused2("BC6H_UF16", b16, 0, 4, 95, s6, "ITW_MIP_SRGB")
refused2("BC6H_SF16", b16, 0, 4, 96, s6, "ITW_MIP_SRGB")
refused2("BC4_SNORM", b8, 0, 4, 81, None, "ITW_MIP_SRGB")
refused2("BC5_SNORM", b8, 0, 4, 84, None, "ITW_MIP_SRGB")
for ops in (1, 2, 4, 7):
    refused2("normal ops %%d" %% ops, b8, ops, 4, 83, None, "not colour")
    refused2("normal ops %%d, BC7_SRGB" %% ops, b8, ops, 5, 99, s7, "not colour")
refused2("unknown mip flag 2", b8, 0, 2, 71, None, "unknown mip flag")
refused2("unknown mip flag 2 beside the flag", b8, 0, 6, 72, None, "unknown mip flag")
refused2("unknown high mip flag", b8, 0, 0x80000000, 71, None, "unknown mip flag")
refused2("what the plain entry refuses: unknown ops", b8, 8, 0, 71, None, "ops bits")
L.itwClearError()
assert L.itwCompressImageMippedEx(b8, 1, 0, 0, 4, None, 71, None, None, None) is False and itw_amd.last_error()      # the plain entry's checks hold: null target
assert not out.any() and (store == 0x11).all()
print("mipped refused", m)
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.split("\n")[:2] == ["generate refused 6", "mipped refused 16"]


# VGPRs (AGPRs included), LDS bytes and scratch bytes of every mip kernel instantiation that existed before the sRGB kind, as the parent
# commit's build reports them (tools/kernel_resources.py over its csrc/build/mipgen.o; the parent's names lack the trailing `false`)
PARENT_FIGURES = {
    "mip_pyramid_kernel<4, false>": (29, 5440, 0),
    "mip_tail_kernel<4, false>": (30, 5120, 0),
    "mip_level_kernel<4, false, false>": (17, 0, 0),
    "mip_level_kernel<4, true, false>": (24, 0, 0),
    "mip_pyramid_kernel<8, false>": (50, 5440, 0),
    "mip_tail_kernel<8, false>": (40, 5120, 0),
    "mip_level_kernel<8, false, false>": (21, 0, 0),
    "mip_level_kernel<8, true, false>": (24, 0, 0),
    "mip_widen_signed_kernel<4>": (16, 0, 0),
    "mip_widen_signed_kernel<8>": (15, 0, 0),
    "mip_widen_signed_kernel<16>": (24, 0, 0),
}
SRGB_KERNELS = ("mip_pyramid_kernel<4, true>", "mip_tail_kernel<4, true>", "mip_level_kernel<4, false, true>", "mip_level_kernel<4, true, true>")


def test_the_old_mip_kernels_keep_their_resources_and_the_new_ones_have_no_scratch():
    obj = os.path.join(CSRC, "build", "mipgen.o")
    if not os.path.exists(obj):
        pytest.skip("csrc/build/ is not populated: run __graft_entry__.build() first")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), obj], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines():
        m = re.match(r"(?:void )?itw::(\S.*?)\s+vgpr\s+(\d+) agpr\s+(\d+) .*?scratch\s+(\d+) B\s+lds\s+(\d+) B\s+spills v(\d+) s(\d+)", line)
        if m:
            table[m.group(1)] = (int(m.group(2)) + int(m.group(3)), int(m.group(5)), int(m.group(4)), int(m.group(6)) + int(m.group(7)))
    assert set(table) == set(PARENT_FIGURES) | set(SRGB_KERNELS), sorted(table)
    for name, want in PARENT_FIGURES.items():
        assert table[name][:3] == want, (name, table[name], want)
    for name in SRGB_KERNELS:
        regs, lds, scratch, spills = table[name]
        assert scratch == 0 and spills == 0, (name, table[name])
        assert lds <= 8192 and regs <= 128, (name, table[name])          # four workgroups a CU and more under both limits (512 registers a lane, 160 KiB)
