"""Volume mip chains without a GPU (include/itw_dispatch.h, "Mip chains: volumes"): the numpy model of tests/_mip3d.py equals every case
the reference's own _Generate3DMips*Filter functions recorded (tests/golden/mip3d_ref.npz, tools/make_mip3d_golden.py) -- which makes it
the yardstick for RGBA8 and sRGB, which the reference does not pin -- the level, slice and layout arithmetic of the library, and every
refusal of the two entry points, which arrives through the error mode before any device work."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _mip3d as M3
import _mip_filters as MF
import _mipgen as M
import _resize as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "intel-texture-works-plugin_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def recording():
    arrays = dict(np.load(os.path.join(GOLD, "mip3d_ref.npz")))
    with open(os.path.join(GOLD, "mip3d_ref_sha256.json")) as f:
        pins = json.load(f)
    return arrays, pins


def _all_cases():
    for c in M3.CASES + M3.SHA_CASES:
        yield c, M3.variants(*c[:3])
    for c in M3.WIDE_BOX_CASES:
        yield c, [("box", "")]


def test_the_recording_is_complete(recording):
    arrays, pins = recording
    names = [M3.case_name(f, wr, w, h, d) for (w, h, d, _), vs in _all_cases() for f, wr in vs]
    assert sorted(pins["cases"]) == sorted(names) and len(names) == 158
    # box is recorded for the powers of two alone (the reference refuses the rest), cubic and triangle under clamp, wrap W and wrap UVW
    assert [c[:3] for c in M3.CASES + M3.SHA_CASES if ("box", "") in M3.variants(*c[:3])] == \
        [(2, 2, 2), (4, 4, 4), (8, 8, 8), (4, 8, 2), (2, 4, 8), (4, 16, 4), (1, 1, 8), (1, 8, 1), (16, 16, 16), (8, 8, 1), (32, 32, 32), (32, 64, 16)]
    assert [wr for f, wr in M3.variants(5, 3, 7) if f == "triangle"] == ["", "w", "uvw"] == [wr for f, wr in M3.variants(5, 3, 7) if f == "cubic"]
    # the wide cases keep the levels above the stale scanline only; every other recorded case keeps every level
    assert pins["cases"]["box_clamp_8x2x4"]["levels"] == [1] and pins["cases"]["box_clamp_16x4x16"]["levels"] == [1, 2]
    for name, e in pins["cases"].items():
        if name not in ("box_clamp_8x2x4", "box_clamp_16x4x16"):
            assert e["levels"] == list(range(1, M3.levels_of(e["width"], e["height"], e["depth"]))), name
        assert e["stored"] == ((e["width"], e["height"], e["depth"], e["seed"]) not in M3.SHA_CASES), name
    assert os.path.getsize(os.path.join(GOLD, "mip3d_ref.npz")) < os.path.getsize(os.path.join(GOLD, "resize_ref.npz"))


@pytest.mark.parametrize("filt", M3.FILTERS)
def test_the_model_equals_every_recorded_case(recording, filt):
    arrays, pins = recording
    seen = 0
    for (w, h, d, seed), vs in _all_cases():
        base = M3.seeded_half_volume(d, h, w, seed)
        for f, wrap in vs:
            if f != filt:
                continue
            name = M3.case_name(f, wrap, w, h, d)
            e = pins["cases"][name]
            assert hashlib.sha256(base.tobytes()).hexdigest() == e["input_sha256"], name
            levels = M3.chain(base, f, wrap, levels=e["levels"][-1] + 1)
            for l in e["levels"]:
                lw, lh, ld = M3.level_size(w, h, d, l)
                assert levels[l].shape == (ld, lh, lw, 4) and levels[l].dtype == np.uint16
                if e["stored"]:
                    assert np.array_equal(levels[l], arrays[f"{name}_l{l}"]), (name, l)
            assert hashlib.sha256(b"".join(levels[l].tobytes() for l in e["levels"])).hexdigest() == e["levels_sha256"], name
            seen += 1
    assert seen == {"box": 14, "point": 18, "linear": 18, "cubic": 54, "triangle": 54}[filt]


def test_the_default_is_box_for_powers_of_two_and_triangle_otherwise():
    assert M3.default_filter(16, 4, 16) == "box" and M3.default_filter(1, 1, 8) == "box"
    for size in ((5, 4, 4), (4, 6, 4), (4, 4, 3), (12, 20, 1)):
        assert M3.default_filter(*size) == "triangle", size
    base = M3.seeded_half_volume(5, 3, 4, 7)
    assert all(np.array_equal(a, b) for a, b in zip(M3.chain(base), M3.chain(base, "triangle")))


def test_the_scalar_scatter_and_the_ranked_form_of_the_triangle_model_agree():
    for (d, h, w), wrap in (((5, 3, 7), ""), ((5, 3, 7), "uvw"), ((2, 4, 4), "w"), ((1, 5, 3), "uv")):
        f = M.widen(M3.seeded_half_volume(d, h, w, 5))
        assert np.array_equal(M3.triangle_unrounded(f, wrap).view(np.uint32), M3.triangle_unrounded_scatter(f, wrap).view(np.uint32)), (d, h, w, wrap)


@pytest.mark.parametrize("kind", M3.KINDS)
def test_a_depth_of_one_is_the_2d_chain_under_every_filter_triangle_included(recording, kind):
    """The recorded 12x20x1 and 8x8x1 cases decide it for RGBA16F: the reference's 3D functions on one slice give the bytes its 2D
    functions give (mipfilter_ref / mipgen_ref pin the 2D model).  Under triangle the z list of 1 -> 1 holds the one weight 1.0f, and
    (1.0f * yw) * xw is yw * xw.  The model says the same for the other two kinds."""
    arrays, _ = recording
    assert [(e, w) for e, w in MF.triangle_lists(1, 1, False)[0]] == [(0, np.float32(1.0))] == [(e, w) for e, w in MF.triangle_lists(1, 1, True)[0]]
    for w, h, seed in ((12, 20, 85), (8, 8, 84)):
        vol = M3.seeded_half_volume(1, h, w, seed) if kind == "rgba16f" else M3.seeded_byte_volume(1, h, w, seed)
        sizes = [M.level_size(w, h, l) for l in range(M.levels_of(w, h))]
        for filt in ("point", "linear", "cubic", "triangle") + (("box",) if M3.default_filter(w, h, 1) == "box" else ()):
            for wrap in (("", "uv") if filt in ("cubic", "triangle") else ("",)):
                flat = R.chain(vol[0], sizes, filt, wrap, kind)
                got = M3.chain(vol, filt, wrap, kind)
                assert len(got) == len(flat) and all(np.array_equal(g[0], f) for g, f in zip(got, flat)), (w, h, filt, wrap)
                if kind == "rgba16f" and wrap == "":
                    name = M3.case_name(filt, "", w, h, 1)
                    assert all(np.array_equal(flat[l], arrays[f"{name}_l{l}"][0]) for l in range(1, len(flat))), name


def test_levels_slices_and_layout(itw):
    """host arithmetic the header states: the binding's own, against the model's and the library's 2D call"""
    L = itw.lib()
    for w, h, d in ((1, 1, 1), (2, 2, 2), (5, 3, 7), (16, 4, 16), (12, 20, 1), (1, 1, 8), (100, 60, 40), (256, 256, 256), (3, 70000, 2)):
        assert itw.mip_levels_3d(w, h, d) == M3.levels_of(w, h, d) == 1 + int(np.floor(np.log2(max(w, h, d)))) == L.itwMipLevels(max(w, h), d)
        full = M3.levels_of(w, h, d)
        for levels in range(0, full + 1):
            n = levels or full
            assert itw.mip_slices_3d(d, n) == M3.slices_of(d, n)
            total, lay = itw.mip_chain_layout_3d(w, h, d, levels, 8)
            want, at = [], 0
            for l in range(n):
                lw, lh, ld = M3.level_size(w, h, d, l)
                for _ in range(ld):
                    want.append((at, lw, lh, lw * 8))
                    at += lw * lh * 8
            assert lay == want and total == at
        with pytest.raises(ValueError):
            itw.mip_chain_layout_3d(w, h, d, full + 1, 4)
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 4, 4)):
        assert itw.mip_levels_3d(*bad) == 0
        with pytest.raises(ValueError):
            itw.mip_chain_layout_3d(*bad)
    assert itw.mip_slices_3d(7, 5) == 7 + 3 + 1 + 1 + 1 and itw.mip_slices_3d(4, 0) == 0
    for bad in ((4, 4, 4, 0, 3), (4, 4, 4, -1, 4), (1 << 29, 1, 1, 1, 8)):                  # pixel_size, levels, a row above 2^31 - 1 bytes
        with pytest.raises(ValueError):
            itw.mip_chain_layout_3d(*bad)
    # the payload of a volume file is the chain calls' stream over the same list
    _, lay = itw.mip_chain_layout_3d(12, 20, 6, 0, 4)
    desc = itw.DdsVolumeDesc(12, 20, 6, 5, 71)
    assert itw.chain_bytes("bc1", [(hh, ww) for _, ww, hh, _ in lay]) == L.itwDdsFileBytes(desc) - L.itwDdsHeaderBytes(desc)


def test_the_library_exports_no_new_function_for_volumes(itw):
    """a volume arrives through a flag bit of the existing calls and a kind of the existing descriptor: no header declares a new function"""
    for header in ("itw_dispatch.h", "itw_dds.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        assert not re.findall(r"\bitw\w*(?:3D|Volume)\w*\s*\(", text), header
    assert not [n for n in itw.EXPORTED_SYMBOLS if "3D" in n or "Volume" in n]


def test_the_flag_constants_agree(itw):
    header = open(os.path.join(ROOT, "include", "itw_dispatch.h")).read()
    assert re.search(r"enum \{ ITW_MIP_WRAP_W = 0x100,", header) and re.search(r"ITW_MIP_VOLUME = 0x8000 \};", header) and (itw.MIP_WRAP_W, itw.MIP_VOLUME) == (0x100, 0x8000)
    assert re.search(r"enum \{ ITW_DDS_VOLUME = 2 \};", open(os.path.join(ROOT, "include", "itw_dds.h")).read()) and itw.DDS_VOLUME == 2
    assert itw.mip_filter_flags_3d("triangle", "uvw", True, True) == 0x20 | 0x40 | 0x80 | 0x100 | 4 | 1
    assert itw.mip_filter_flags_3d("point") == 0x400 and itw.mip_filter_flags_3d("linear", "w") == 0x900 and itw.mip_filter_flags_3d("cubic") == 0x10
    with pytest.raises(ValueError):
        itw.mip_filter_flags_3d("box")
    with pytest.raises(ValueError):
        itw.mip_filter_flags_3d(None, "x")


def test_refusals_in_a_fresh_interpreter():
    """Fresh interpreter: the error mode is process-wide.  Every refusal leaves its message, returns -1 / false and changes no byte; it
    happens on a machine without a GPU as well, so before any device work.  A call the checks accept goes on to the device: it succeeds
    where there is one and fails for that reason alone where there is none."""
    code = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
import itw_amd
L = itw_amd.lib()
S = itw_amd.RgbaSurface
itw_amd.set_error_mode(itw_amd.ON_ERROR_RETURN)
store = np.full(1 << 16, 0x11, np.uint8)
p = store.ctypes.data
def volume(w, h, d, levels, px=4):
    out, at, i = (S * sum(max(1, d >> l) for l in range(levels)))(), 0, 0
    for l in range(levels):
        lw, lh = max(1, w >> l), max(1, h >> l)
        for z in range(max(1, d >> l)):
            out[i] = S(p + at, lw, lh, lw * px)
            at += lw * lh * px
            i += 1
    assert at <= store.size
    return out
def ptr(a):
    return C.cast(a, C.c_void_p)
n = 0
def refused(what, call, *words):
    global n
    L.itwClearError()
    assert call() in (-1, False), what
    for word in words:
        assert word in itw_amd.last_error(), (what, itw_amd.last_error())
    n += 1
PL, SR, CU, TR, WU, WV, WW, RS, PT, LN, MU, MV, VOL = 1, 4, 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x400, 0x800, 0x1000, 0x2000, 0x8000
def gen(slices, depth, levels, px, flags):
    return lambda: L.itwGenerateMipChain(ptr(slices), depth, levels, px, flags | VOL)
for px in (4, 8):
    v = volume(8, 8, 4, 4, px)
    for a, b in ((PT, LN), (PT, CU), (PT, TR), (LN, CU), (LN, TR), (CU, TR), (PT, LN | CU)):
        refused("two filters", gen(v, 4, 4, px, a | b), "two filter bits together", "one of ITW_MIP_POINT")
    refused("resize", gen(v, 4, 4, px, RS), "ITW_MIP_RESIZE", "no 3D resize")
    refused("resize beside a filter", gen(v, 4, 4, px, RS | CU), "ITW_MIP_RESIZE")
    for bit in (MU, MV, MU | CU):
        refused("mirror", gen(v, 4, 4, px, bit), "ITW_MIP_MIRROR")
    for bits in (2, 8, 0x4000, 0x80000000, 2 | TR):
        refused("bit 0x%%x" %% bits, gen(v, 4, 4, px, bits), "unknown flag bits")
    refused("five levels of 8 x 8 x 4", gen(v, 4, 5, px, 0), "5 levels", "8 x 8 x 4 has 4")
    refused("negative depth", gen(v, -1, 2, px, 0), "depth -1")
    refused("null slices", gen(None, 4, 2, px, 0), "null slices")
    bad = volume(8, 8, 4, 4, px); bad[4].width = 3
    refused("a level that is not the definition's", gen(bad, 4, 4, px, TR), "level 1 slice 0", "the chain's is 4 x 4")
    bad = volume(8, 8, 4, 4, px); bad[5].height = 8
    refused("a slice that is not its level's", gen(bad, 4, 4, px, 0), "level 1 slice 1")
    bad = volume(8, 8, 4, 4, px); bad[2].width = 4
    refused("a base slice of another size", gen(bad, 4, 4, px, 0), "level 0 slice 2")
    bad = volume(8, 8, 4, 4, px); bad[6].stride = 2 * px - 1
    refused("a stride below the row", gen(bad, 4, 4, px, CU), "level 2 slice 0")
    bad = volume(8, 8, 4, 4, px); bad[3].ptr = None
    refused("null texels", gen(bad, 4, 4, px, 0), "level 0 slice 3")
    bad = volume(8, 8, 4, 4, px); bad[1].ptr = p + 1
    refused("misaligned texels", gen(bad, 4, 4, px, 0), "level 0 slice 1")
    zero = volume(8, 8, 4, 2, px); zero[0].width = 0
    refused("a base of width 0", gen(zero, 4, 2, px, 0), "0 x 8 x 4")
refused("pixel_size 3", gen(volume(8, 8, 4, 4), 4, 4, 3, 0), "pixel_size 3")
refused("sRGB halves", gen(volume(8, 8, 4, 4, 8), 4, 4, 8, SR), "ITW_MIP_SRGB")
refused("more slices than a launch covers", gen(volume(1, 1, 8, 2), 131072, 2, 4, 0), "131072 slices", "131 071")
assert (store == 0x11).all()
print("generate refused", n)

# without ITW_MIP_VOLUME every call keeps refusing 0x100 as unknown, and the alpha calls refuse the volume bit itself
m = 0
img = np.zeros((8, 8, 4), np.uint8)
out = np.full(4096, 0x33, np.uint8)
b8, t = ptr((S * 1)(S(img.ctypes.data, 8, 8, 32))), out.ctypes.data
two = (S * 2)(S(p, 8, 8, 32), S(p + 256, 4, 4, 16))
for bits in (WW, WW | TR, WW | RS | CU):
    L.itwClearError()
    assert L.itwGenerateMipChain(ptr(two), 1, 2, 4, bits) == -1 and "unknown flag" in itw_amd.last_error(), bits
    L.itwClearError()
    assert L.itwCompressImageMippedEx(b8, 1, 0, 0, bits, t, 71, None, None, None) is False and "unknown mip flag" in itw_amd.last_error(), bits
    m += 2
for bits in (VOL, VOL | WW, VOL | TR):
    L.itwClearError()
    assert L.itwGenerateMipChainAlpha(ptr(two), 1, 2, bits, None, None) == -1 and "unknown flag" in itw_amd.last_error(), bits
    L.itwClearError()
    assert L.itwCompressImageMippedAlpha(b8, 1, 0, bits, None, t, 71, None, None, None) is False and "unknown mip flag" in itw_amd.last_error(), bits
    m += 2
print("2D calls refused", m)

# the one-call save: the flag rules, the chain call's own, and its own
k = 0
vol = np.zeros((4, 8, 8, 4), np.uint8)
half = np.zeros((4, 8, 8, 4), np.uint16)
def slices(a, px):
    return ptr((S * len(a))(*[S(a[z].ctypes.data, a.shape[2], a.shape[1], a.shape[2] * px) for z in range(len(a))]))
def save(sl, depth, levels, flags, fmt, settings=None, target=t):
    return lambda: L.itwCompressImageMippedEx(sl, depth, levels, 0, flags | VOL, target, fmt, settings, None, None)
def refused_save(what, call, *words):
    global k
    L.itwClearError()
    assert call() is False, what
    for word in words:
        assert word in itw_amd.last_error(), (what, itw_amd.last_error())
    k += 1
refused_save("unknown bit", save(slices(vol, 4), 4, 0, 2, 71), "unknown mip flag bits")
refused_save("normal ops", lambda: L.itwCompressImageMippedEx(slices(vol, 4), 4, 0, 4, VOL, t, 71, None, None, None), "normal ops 0x4 with ITW_MIP_VOLUME")
refused_save("resize", save(slices(vol, 4), 4, 0, RS, 71), "ITW_MIP_RESIZE")
refused_save("mirror", save(slices(vol, 4), 4, 0, MU | CU, 71), "ITW_MIP_MIRROR")
refused_save("two filters", save(slices(vol, 4), 4, 0, CU | TR, 71), "two filter bits together")
refused_save("sRGB with BC6H", save(slices(half, 8), 4, 0, SR, 95, C.cast(C.byref(itw_amd.bc6h_profile("fast")), C.c_void_p)), "ITW_MIP_SRGB", "RGBA16F")
refused_save("sRGB with BC4S", save(slices(vol, 4), 4, 0, SR, 81), "ITW_MIP_SRGB", "signed")
refused_save("five levels", save(slices(vol, 4), 4, 5, 0, 71), "5 levels", "8 x 8 x 4 has 4")
refused_save("negative levels", save(slices(vol, 4), 4, -1, 0, 71), "-1 levels")
refused_save("no slices", save(slices(vol, 4), 0, 0, 0, 71), "0 images")
refused_save("null target", save(slices(vol, 4), 4, 0, 0, 71, None, None), "null")
refused_save("BC7 without settings", save(slices(vol, 4), 4, 0, 0, 98), "settings")
refused_save("an unknown format", save(slices(vol, 4), 4, 0, 0, 70), "70")
refused_save("the signed BC6H decode code", save(slices(half, 8), 4, 0, 0, 0x8E8E), "decode code")
odd = (S * 4)(*[S(vol[z].ctypes.data, 8, 8 if z != 2 else 4, 32) for z in range(4)])
refused_save("slices of two sizes", save(ptr(odd), 4, 0, 0, 71), "slice 2 is 8 x 4")
assert (out == 0x33).all() and (store == 0x11).all()
print("save refused", k)

# nothing to do stays 0 whatever the machine
assert L.itwGenerateMipChain(ptr(volume(8, 8, 4, 1)), 4, 1, 4, VOL | TR | WW) == 0 and L.itwGenerateMipChain(ptr(volume(8, 8, 4, 2)), 0, 2, 4, VOL) == 0
assert L.itwGenerateMipChain(None, 4, 0, 4, VOL | PT) == 0
assert (store == 0x11).all()
# what the checks accept: every filter by name without the resize bit, the three wrap bits beside every filter, per_level, sRGB codes
accepted = [((8, 8, 4), 0), ((8, 8, 4), PT), ((8, 8, 4), LN | WU | WV | WW), ((8, 8, 4), CU | WW), ((8, 8, 4), TR | WU | WV | WW), ((8, 8, 4), PL | SR),
            ((5, 3, 7), 0), ((5, 3, 7), PT | WW), ((12, 20, 1), CU), ((1, 1, 8), WW)]
for (w, h, d), flags in accepted:
    levels = itw_amd.mip_levels_3d(w, h, d)
    L.itwClearError()
    rc = L.itwGenerateMipChain(ptr(volume(w, h, d, levels)), d, levels, 4, flags | VOL)
    if itw_amd.available():
        assert rc == 0, ((w, h, d), hex(flags), itw_amd.last_error())
    else:
        assert rc == -1, ((w, h, d), hex(flags))
        assert "unknown" not in itw_amd.last_error() and "ITW_MIP" not in itw_amd.last_error() and "level" not in itw_amd.last_error(), itw_amd.last_error()
if not itw_amd.available():
    assert (store == 0x11).all()
print("accepted: ran" if itw_amd.available() else "accepted: by the checks")
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.split("\n")
    assert lines[:3] == ["generate refused 57", "2D calls refused 12", "save refused 15"], lines
    assert lines[3] in ("accepted: ran", "accepted: by the checks")


def test_the_volume_kernels_have_no_scratch_and_no_spills():
    obj = os.path.join(CSRC, "build", "mip3d.o")
    if not os.path.exists(obj):
        pytest.skip("csrc/build/ is not populated: run __graft_entry__.build() first")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), obj], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines():
        m = re.match(r"(?:void )?itw::(\S.*?)\s+vgpr\s+(\d+) agpr\s+(\d+) .*?scratch\s+(\d+) B\s+lds\s+(\d+) B\s+spills v(\d+) s(\d+)", line)
        if m:
            table[m.group(1)] = (int(m.group(2)) + int(m.group(3)), int(m.group(5)), int(m.group(4)), int(m.group(6)) + int(m.group(7)))
    kinds = ("4, false", "4, true", "8, false")
    want = {f"mip3d_{f}_kernel<{k}>" for k in kinds for f in M3.FILTERS}
    assert set(table) == want, sorted(table)
    for name, (regs, lds, scratch, spills) in table.items():
        assert scratch == 0 and spills == 0, (name, table[name])
        assert regs <= 128 and lds <= 2052, (name, table[name])          # four waves a SIMD by registers at the least; the sRGB tables and nothing else in LDS
