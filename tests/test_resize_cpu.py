"""The free-size chain without a GPU (include/itw_dispatch.h, "Mip chains: free sizes", ITW_MIP_RESIZE): the numpy model of tests/_resize.py
against the reference's own functions as tests/golden/resize_ref.npz records them (tools/make_resize_golden.py), the library's host tables
against the same recording, every refusal before any device work, the flag constants, fit_size against a table worked out by hand, the
product's symbol list, and the scratch and spills of csrc/build/resize.o.  Every comparison is == on every byte."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _mip_filters as MF
import _resize as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "intel-texture-works-plugin_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden")
SMALL = 4096
LINEAR_TABLE = np.dtype([("u", "<i4", 2), ("w", "<f4", 2)])
CUBIC_TABLE = np.dtype([("u", "<i4", 4), ("x", "<f4")])
TRIANGLE_TABLE = np.dtype([("idx", "<i4", 2), ("w", "<f4")])
DTYPES = {"linear": LINEAR_TABLE, "cubic": CUBIC_TABLE, "triangle": TRIANGLE_TABLE}


@pytest.fixture(scope="module")
def recording():
    arrays = dict(np.load(os.path.join(GOLD, "resize_ref.npz")))
    with open(os.path.join(GOLD, "resize_ref_sha256.json")) as f:
        pins = json.load(f)
    return arrays, pins


def _table_bytes(kind, idx, wgt):
    rec = np.zeros(len(idx), dtype=DTYPES[kind])
    rec["idx" if kind == "triangle" else "u"] = idx
    rec["x" if kind == "cubic" else "w"] = wgt
    return rec.tobytes()


def _recorded_tables():
    for source, dest in R.table_pairs():
        for kind, address in R.TABLE_VARIANTS:
            if kind == "linear" and address == R.WRAP and dest >= source > 1:
                continue                                           # the library refuses it: not recorded
            yield kind, address, source, dest


def _model_table(kind, address, source, dest):
    if kind == "linear":
        u0, w0, u1, w1 = R.linear_filter(source, dest, address == R.WRAP)
        return np.stack([u0, u1], axis=1).astype(np.int32), np.stack([w0, w1], axis=1)
    if kind == "cubic":
        taps, x = R.cubic_filter(source, dest, address)
        return taps.astype(np.int32), x
    return MF.triangle_table(source, dest, address == R.WRAP)


def test_the_recording_is_complete(recording):
    arrays, pins = recording
    names = [R.case_name(f, a, sizes) for sizes, _ in R.CASES for f, a in R.variants(sizes)]
    assert sorted(pins["cases"]) == sorted(names) and len(names) == 223
    assert sorted(pins["tables"]) == sorted(R.table_name(k, a, s, d) for k, a, s, d in _recorded_tables())
    by_size = {R.sizes_name(sizes): seed for sizes, seed in R.CASES}
    for name, e in pins["cases"].items():
        sizes = [tuple(s) for s in e["sizes"]]
        assert e["seed"] == by_size[R.sizes_name(sizes)] and e["stored"] == [int(w * h <= SMALL) for w, h in sizes[1:]], name
    # the issue's table: box where the ratio is exactly 2:1 and nowhere else, linear-wrap left out where the call refuses it, mirror under cubic only
    assert [R.sizes_name(s) for s, _ in R.CASES if ("box", "") in R.variants(s)] == ["16x16_8x8"]
    assert ("linear", "u") not in R.variants(((4, 4), (8, 8))) and ("linear", "v") in R.variants(((3, 5), (7, 4))) and ("linear", "u") not in R.variants(((3, 5), (7, 4)))
    assert ("linear", "uv") in R.variants(((1, 1), (4, 4))) and ("linear", "uv") in R.variants(((16, 16), (8, 8)))
    assert [f for f, a in R.variants(((7, 7), (3, 3))) if a == "mirror"] == ["cubic"]
    # no recorded triangle table leaves a destination without an entry (the header says what the library writes if one did)
    assert all(e["destinations_without_entry"] == 0 for n, e in pins["tables"].items() if n.startswith("triangle"))


@pytest.mark.parametrize("filt", R.FILTERS)
def test_the_model_equals_every_recorded_case(recording, filt):
    arrays, pins = recording
    seen = 0
    for sizes, seed in R.CASES:
        base = MF.seeded_half_image(sizes[0][1], sizes[0][0], seed)
        for f, addr in R.variants(sizes):
            if f != filt:
                continue
            name = R.case_name(f, addr, sizes)
            e = pins["cases"][name]
            assert hashlib.sha256(base.tobytes()).hexdigest() == e["input_sha256"], name
            levels = R.chain(base, sizes, f, addr)[1:]
            for i, lv in enumerate(levels):
                assert lv.shape == (sizes[i + 1][1], sizes[i + 1][0], 4)
                if e["stored"][i]:
                    assert np.array_equal(lv, arrays[f"{name}_l{i + 1}"]), (name, i + 1)
            assert hashlib.sha256(b"".join(lv.tobytes() for lv in levels)).hexdigest() == e["levels_sha256"], name
            seen += 1
    assert seen == {"point": 56, "box": 4, "linear": 37, "cubic": 70, "triangle": 56}[filt]


def test_the_default_filter_is_box_at_exactly_two_to_one_and_linear_elsewhere(recording):
    arrays, pins = recording
    for sizes, want in ((((16, 16), (8, 8)), "box"), (((7, 7), (3, 3)), "linear"), (((4, 4), (8, 8)), "linear"), (((20, 12), (33, 7), (8, 8)), "linear")):
        seed = dict((R.sizes_name(s), k) for s, k in R.CASES)[R.sizes_name(sizes)]
        base = MF.seeded_half_image(sizes[0][1], sizes[0][0], seed)
        got = R.chain(base, sizes, None, "")[1:]
        assert hashlib.sha256(b"".join(lv.tobytes() for lv in got)).hexdigest() == pins["cases"][R.case_name(want, "", sizes)]["levels_sha256"]
    assert R.pair_filter(None, 16, 8, 8, 8) == "linear" and R.pair_filter(None, 2, 2, 1, 1) == "box" and R.pair_filter("point", 2, 2, 1, 1) == "point"


def test_the_scalar_scatter_and_the_ranked_form_of_the_triangle_model_agree():
    for (w, h), (dw, dh), seed in (((3, 5), (7, 4), 1), ((7, 7), (3, 3), 2), ((12, 20), (5, 2), 3), ((9, 4), (2, 9), 4)):
        f = MF.widen(MF.seeded_half_image(h, w, seed), "rgba16f")
        for wrap in MF.WRAPS:
            a, b = R.triangle_unrounded_scatter(f, dw, dh, "u" in wrap, "v" in wrap), R.triangle_unrounded(f, dw, dh, "u" in wrap, "v" in wrap)
            assert a.tobytes() == b.tobytes(), (w, h, dw, dh, wrap)


def test_the_model_equals_every_recorded_table(recording):
    arrays, pins = recording
    n = 0
    for kind, address, source, dest in _recorded_tables():
        name = R.table_name(kind, address, source, dest)
        idx, wgt = _model_table(kind, address, source, dest)
        e = pins["tables"][name]
        assert len(idx) == e["entries"], name
        assert np.array_equal(idx, arrays[name + "_i"]) and wgt.tobytes() == arrays[name + "_w"].tobytes(), name
        assert hashlib.sha256(_table_bytes(kind, idx, wgt)).hexdigest() == e["sha256"], name
        n += 1
    assert n == len(pins["tables"])
    # the point index against the reference's running sum, and its bound
    for source, dest in R.table_pairs() + [(4000, 4096), (16384, 3), (3, 16384)]:
        inc, sx, want = (source << 16) // dest, 0, []
        for _ in range(dest):
            want.append(sx >> 16)
            sx += inc
        got = R.point_index(source, dest)
        assert got.tolist() == want and got.max() < source


def test_an_upscale_gives_small_negative_cubic_x_and_mirror_differs_from_clamp_two_texels_out():
    taps, x = R.cubic_filter(4, 8, R.CLAMP)
    assert x[0] < 0 and taps[0].tolist() == [0, 0, 1, 2]          # (ptrdiff_t)(-0.25f) is 0
    clamp, mirror, wrap = (R.cubic_filter(4, 8, a)[0] for a in (R.CLAMP, R.MIRROR, R.WRAP))
    assert clamp[-1].tolist() == [2, 3, 3, 3] and mirror[-1].tolist() == [2, 3, 3, 2] and wrap[-1].tolist() == [2, 3, 0, 1]
    assert mirror[0].tolist() == [0, 0, 1, 2] and wrap[0].tolist() == [3, 0, 1, 2]
    # at ratios >= 1 mirror is clamp: why the chain's filters have no such bit
    for source, dest in ((8, 4), (7, 3), (130, 3), (64, 16)):
        assert np.array_equal(R.cubic_filter(source, dest, R.MIRROR)[0], R.cubic_filter(source, dest, R.CLAMP)[0])


def test_the_linear_wrap_artefact_is_what_the_header_says_and_is_not_recorded():
    u0, w0, u1, w1 = R.linear_filter(4, 8, True)
    assert (int(u0[-1]), int(u1[-1]), float(w0[-1]), float(w1[-1])) == (3, 0, -3.25, 4.25)
    # on a shrinking axis the wrap branches do not fire on any recorded pair
    for source, dest in R.table_pairs():
        if dest < source:
            a, b = R.linear_filter(source, dest, True), R.linear_filter(source, dest, False)
            assert all(np.array_equal(p, q) for p, q in zip(a, b)), (source, dest)


def test_the_librarys_host_tables_equal_the_recorded_ones(itw, recording):
    """itwTestResizeTable and itwTestMipFilterTable (libispc_texcomp_test.so only): csrc/mip_filters.hpp's builders, the ones the kernels and
    the entry point use -- a linear table, a mirror-cubic table and the triangle lists of upscale pairs among them."""
    arrays, pins = recording
    T = itw.test_lib()
    assert not hasattr(itw.lib(), "itwTestResizeTable")
    seen = set()
    for kind, address, source, dest in _recorded_tables():
        name = R.table_name(kind, address, source, dest)
        e = pins["tables"][name]
        if kind == "triangle":
            cap = 8 * max(source, dest) + 16
            idx, wgt = np.full((cap, 2), -7, np.int32), np.full(cap, -7.0, np.float32)
            n = T.itwTestMipFilterTable(2, source, dest, address, idx.ctypes.data, wgt.ctypes.data, cap)
        else:
            cap, per = dest + 3, 2 if kind == "linear" else 4
            idx = np.full((cap, per), -7, np.int32)
            wgt = np.full((cap, 2) if kind == "linear" else cap, -7.0, np.float32)
            n = T.itwTestResizeTable(4 if kind == "linear" else 1, source, dest, address, idx.ctypes.data, wgt.ctypes.data, cap)
        assert n == e["entries"], (name, n)
        assert hashlib.sha256(_table_bytes(kind, idx[:n], wgt[:n])).hexdigest() == e["sha256"], name
        assert (idx[n:] == -7).all() and (wgt[n:] == -7.0).all(), name
        seen.add((kind, address, dest > source))
    assert {("linear", R.CLAMP, True), ("cubic", R.MIRROR, True), ("cubic", R.WRAP, True), ("triangle", R.CLAMP, True), ("triangle", R.WRAP, True)} <= seen
    for source, dest in R.table_pairs():                           # the point index; mirror is clamp for linear
        idx, wgt = np.full(dest, -7, np.int32), np.zeros(dest, np.float32)
        assert T.itwTestResizeTable(3, source, dest, 0, idx.ctypes.data, wgt.ctypes.data, dest) == dest
        assert np.array_equal(idx, R.point_index(source, dest)) and (wgt == 1).all()
        a, b = (np.zeros((dest, 2), np.int32), np.zeros((dest, 2), np.float32)), (np.zeros((dest, 2), np.int32), np.zeros((dest, 2), np.float32))
        assert T.itwTestResizeTable(4, source, dest, 2, a[0].ctypes.data, a[1].ctypes.data, dest) == dest
        assert T.itwTestResizeTable(4, source, dest, 0, b[0].ctypes.data, b[1].ctypes.data, dest) == dest
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
    small = np.zeros((1, 4), np.int32)
    for bad in ((1, 12, 6, 0, 5), (1, 12, 6, 3, 6), (2, 12, 6, 0, 6), (4, 0, 6, 0, 6), (3, 6, 0, 0, 6)):
        assert T.itwTestResizeTable(*bad[:4], small.ctypes.data, np.zeros(1, np.float32).ctypes.data, bad[4]) == -1, bad


def test_the_flag_constants_agree(itw):
    header = open(os.path.join(ROOT, "include", "itw_dispatch.h")).read()
    assert re.search(r"enum \{ ITW_MIP_RESIZE = 0x200, ITW_MIP_POINT = 0x400, ITW_MIP_LINEAR = 0x800, ITW_MIP_MIRROR_U = 0x1000, ITW_MIP_MIRROR_V = 0x2000 \};", header)
    assert (itw.MIP_RESIZE, itw.MIP_POINT, itw.MIP_LINEAR, itw.MIP_MIRROR_U, itw.MIP_MIRROR_V) == (0x200, 0x400, 0x800, 0x1000, 0x2000)
    assert itw.resize_flags() == 0x200 and itw.resize_flags("point") == 0x600 and itw.resize_flags("linear", "v") == 0xA80
    assert itw.resize_flags("cubic", "u", "uv", True) == 0x200 | 0x10 | 0x40 | 0x3000 | 4 and itw.resize_flags("triangle", mirror="v") == 0x2220
    for bad in (("box",), ("cubic", "w"), ("cubic", "", "vu")):
        with pytest.raises(ValueError):
            itw.resize_flags(*bad)
    # the chain's own flag helper still knows two filters and no new bit
    with pytest.raises(ValueError):
        itw.mip_filter_flags("point")


def test_fit_size_against_a_table_written_out_by_hand(itw):
    """pow2 (texconv's FitPowerOf2 with maxsize 16384): the longer axis becomes the largest power of two <= itself; the other axis the
    power of two y minimising |x / y - w / h|.  4000 x 3000: x = 2048, aspect 1.333; y = 2048 gives 1 (off by .333), 1024 gives 2 (off by
    .667), 4096 gives .5 (off by .833) -> 2048.  300 x 300: 256, ratio 1 exactly.  1 x 7: y = 4, aspect .1429; x = 1 gives .25 (off by
    .107), x = 2 gives .5 -> 1.  16385 x 3: x = 16384, aspect 5461.67; y = 4 gives 4096 (off by 1365.7), y = 2 gives 8192 (off by 2730.3),
    y = 8 gives 2048 (off by 3413.7) -> 4."""
    table = {
        "pow2":      {(4000, 3000): (2048, 2048), (300, 300): (256, 256), (1, 7): (1, 4), (16385, 3): (16384, 4)},
        "pow2_up":   {(4000, 3000): (4096, 4096), (300, 300): (512, 512), (1, 7): (1, 8), (16385, 3): (16384, 4)},
        "multiple4": {(4000, 3000): (4000, 3000), (300, 300): (300, 300), (1, 7): (4, 8), (16385, 3): (16384, 4)},
    }
    for rule, rows in table.items():
        for (w, h), want in rows.items():
            assert itw.fit_size(w, h, rule) == want, (rule, w, h)
    assert itw.fit_size(16385, 3, "pow2_up", max_size=32768) == (32768, 4) and itw.fit_size(16385, 3, "multiple4", max_size=32768) == (16388, 4)
    assert itw.fit_size(4000, 3000, "pow2", max_size=1024) == (1024, 1024) and itw.fit_size(512, 512, "pow2") == (512, 512)
    for bad in ((0, 4, "pow2"), (4, 4, "pow3")):
        with pytest.raises(ValueError):
            itw.fit_size(*bad)


def test_the_product_library_lists_exactly_the_symbols_it_listed_before(itw):
    """The resize arrives through flag bits of itwGenerateMipChain: 132 exported functions, the same names."""
    out = subprocess.run(["nm", "-D", "--defined-only", itw.lib_path()], check=True, capture_output=True, text=True).stdout
    names = sorted(l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T")
    assert names == sorted(itw.EXPORTED_SYMBOLS) and len(names) == 132
    assert hashlib.sha256(("\n".join(names) + "\n").encode()).hexdigest() == "c95d9d1b784b2eba98e5209b41d4654268a44bb0ff28699e20a7fcae01dad85c"


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
def chain(sizes, px=4, items=1):
    out, at = (S * (items * len(sizes)))(), 0
    for i in range(items):
        for l, (w, h) in enumerate(sizes):
            out[i * len(sizes) + l] = S(p + at, w, h, w * px)
            at += max(w, 1) * max(h, 1) * px
    assert at <= store.size
    return out
def ptr(a):
    return C.cast(a, C.c_void_p)
def opts(*a, **k):
    o = itw_amd.MipAlpha(*a, **k)
    return o, C.cast(C.byref(o), C.c_void_p)
n = 0
def refused(what, call, *words):
    global n
    L.itwClearError()
    assert call() in (-1, False), what
    for word in words:
        assert word in itw_amd.last_error(), (what, itw_amd.last_error())
    n += 1
RS, PT, LN, CU, TR, WU, WV, MU, MV = 0x200, 0x400, 0x800, 0x10, 0x20, 0x40, 0x80, 0x1000, 0x2000
up, down = [(4, 4), (8, 8)], [(8, 8), (3, 5)]
def gen(images, items, levels, px, flags):
    return lambda: L.itwGenerateMipChain(ptr(images), items, levels, px, flags)
for px in (4, 8):
    for a, b in ((PT, LN), (PT, CU), (PT, TR), (LN, CU), (LN, TR), (PT, LN | CU)):
        refused("two filters", gen(chain(down, px), 1, 2, px, RS | a | b), "two filter bits together", "one of ITW_MIP_POINT")
    refused("cubic and triangle", gen(chain(down, px), 1, 2, px, RS | CU | TR), "ITW_MIP_CUBIC and ITW_MIP_TRIANGLE together")
    for bit, name in ((PT, "ITW_MIP_POINT"), (LN, "ITW_MIP_LINEAR"), (MU, "ITW_MIP_MIRROR"), (MV, "ITW_MIP_MIRROR"), (MU | CU, "ITW_MIP_MIRROR"), (PT | WU, "ITW_MIP_POINT")):
        refused("0x%%x without the resize bit" %% bit, gen(chain([(8, 8), (4, 4)], px), 1, 2, px, bit), name, "without ITW_MIP_RESIZE")
    for bits in (2, 8, 0x100, 0x4000, 0x80000000):
        for beside in (RS, RS | PT, RS | CU | MU):
            refused("bit 0x%%x beside 0x%%x" %% (bits, beside), gen(chain(down, px), 1, 2, px, bits | beside), "unknown flag")
    # the linear filter's wrap branches on a growing axis, named or by default; the message names the filters that wrap at any ratio
    for flags in (RS | LN | WU, RS | WU, RS | WV, RS | LN | WU | WV, RS | WV | MU):
        refused("linear wrap 0x%%x" %% flags, gen(chain(up, px), 1, 2, px, flags), "linear filter with ITW_MIP_WRAP", "ITW_MIP_CUBIC and ITW_MIP_TRIANGLE wrap")
    refused("linear wrap at equal size", gen(chain([(5, 3), (5, 3)], px), 1, 2, px, RS | WU), "5 texels become 5")
    refused("linear wrap on the second pair of a chain", gen(chain([(16, 16), (8, 8), (8, 9)], px), 1, 3, px, RS | WV), "level 2", "8 texels become 9")
    refused("33 levels", gen(chain([(2, 2)] * 33, px), 1, 33, px, RS), "33 levels", "2 .. 32")
    for size in ((0, 4), (4, 0), (-1, 4)):
        refused("a level of %%r" %% (size,), gen(chain([(4, 4), size], px), 1, 2, px, RS | PT), "level 1", "at least one texel")
    refused("a base of 0 x 0", gen(chain([(0, 0), (4, 4)], px), 1, 2, px, RS), "level 0")
    two = chain(down, px, items=2); two[3].width = 4
    refused("items disagree on level 1", gen(two, 2, 2, px, RS | TR), "item 1 level 1", "one size across the items")
    two = chain(down, px, items=2); two[2].height = 7
    refused("items disagree on the base", gen(two, 2, 2, px, RS), "item 1 level 0")
    short = chain(down, px); short[1].stride = 3 * px - 1
    refused("a stride below the row", gen(short, 1, 2, px, RS | CU), "level 1")
refused("sRGB halves", gen(chain(down, 8), 1, 2, 8, RS | 4), "ITW_MIP_SRGB")
assert (store == 0x11).all()
print("generate refused", n)

# every other call refuses the five bits as unknown
img = np.zeros((8, 8, 4), np.uint8)
out = np.full(4096, 0x33, np.uint8)
b8, t = ptr((S * 1)(S(img.ctypes.data, 8, 8, 32))), out.ctypes.data
m = 0
for bit in (RS, PT, LN, MU, MV, RS | PT, RS | CU | MU):
    L.itwClearError()
    assert L.itwGenerateMipChainAlpha(ptr(chain([(8, 8), (4, 4)])), 1, 2, bit, opts(0, 128)[1], None) == -1 and "unknown flag" in itw_amd.last_error(), bit
    L.itwClearError()
    assert L.itwGenerateMipChainAlpha(ptr(chain([(8, 8), (4, 4)])), 1, 2, bit, None, None) == -1 and "unknown flag" in itw_amd.last_error(), bit
    L.itwClearError()
    assert L.itwCompressImageMippedEx(b8, 1, 0, 0, bit, t, 71, None, None, None) is False and "unknown mip flag" in itw_amd.last_error(), bit
    L.itwClearError()
    assert L.itwCompressImageMippedAlpha(b8, 1, 0, bit, opts(0, 128)[1], t, 77, None, None, None) is False and "unknown mip flag" in itw_amd.last_error(), bit
    m += 4
assert (out == 0x33).all() and (store == 0x11).all()
print("other calls refused", m)

# nothing to do stays 0 whatever the machine
assert L.itwGenerateMipChain(ptr(chain(up)), 1, 1, 4, RS | PT) == 0 and L.itwGenerateMipChain(ptr(chain(up)), 0, 2, 4, RS | MU) == 0
assert L.itwGenerateMipChain(None, 1, 0, 4, RS) == 0
assert (store == 0x11).all()
# what the checks accept: mirror beside every filter, wrap on shrinking axes and on a source of one texel, per_level, 32 levels
accepted = [(down, RS | MU | MV), (down, RS | PT | MU), (down, RS | LN | WU | WV | MV), (down, RS | TR | MU | WU), (down, RS | CU | MU | WU), (down, RS | 1),
            ([(1, 1), (4, 4)], RS | LN | WU | WV), ([(1, 8), (4, 4)], RS | WU), (up, RS | CU | WU | WV), (up, RS | TR | WU | WV), ([(2, 2)] * 32, RS | PT)]
if itw_amd.available():
    for sizes, flags in accepted:
        L.itwClearError()
        assert L.itwGenerateMipChain(ptr(chain(sizes)), 1, len(sizes), 4, flags) == 0, (sizes, hex(flags), itw_amd.last_error())
    print("accepted: ran")
else:
    for sizes, flags in accepted:
        L.itwClearError()
        assert L.itwGenerateMipChain(ptr(chain(sizes)), 1, len(sizes), 4, flags) == -1, (sizes, hex(flags))
        assert "unknown" not in itw_amd.last_error() and "ITW_MIP" not in itw_amd.last_error() and "level" not in itw_amd.last_error(), itw_amd.last_error()
    assert (store == 0x11).all()
    print("accepted: by the checks")
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.split("\n")
    assert lines[:2] == ["generate refused 87", "other calls refused 28"], lines
    assert lines[2] in ("accepted: ran", "accepted: by the checks")


def test_the_resize_kernels_have_no_scratch_and_no_spills():
    obj = os.path.join(CSRC, "build", "resize.o")
    if not os.path.exists(obj):
        pytest.skip("csrc/build/ is not populated: run __graft_entry__.build() first")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), obj], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines():
        m = re.match(r"(?:void )?itw::(\S.*?)\s+vgpr\s+(\d+) agpr\s+(\d+) .*?scratch\s+(\d+) B\s+lds\s+(\d+) B\s+spills v(\d+) s(\d+)", line)
        if m:
            table[m.group(1)] = (int(m.group(2)) + int(m.group(3)), int(m.group(5)), int(m.group(4)), int(m.group(6)) + int(m.group(7)))
    kinds = ("4, false", "4, true", "8, false")
    want = {f"resize_level_kernel<{k}, {m}>" for k in kinds for m in (0, 1, 2)} | {f"resize_cubic_kernel<{k}>" for k in kinds}
    assert set(table) == want, sorted(table)
    for name, (regs, lds, scratch, spills) in table.items():
        assert scratch == 0 and spills == 0, (name, table[name])
        assert regs <= 128 and lds <= 2052, (name, table[name])          # four waves a SIMD by registers at the least; the sRGB tables and nothing else in LDS
