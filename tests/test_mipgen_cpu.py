"""Mip chains without a GPU (include/itw_dispatch.h, "Mip chains"): the numpy model of tests/_mipgen.py equals the recorded outputs of the
reference's own _Generate2DMipsBoxFilter, _Generate2DMipsLinearFilter and _CreateLinearFilter (tests/golden/mipgen_ref.npz and
mipgen_ref_sha256.json, recorded by tools/make_mipgen_golden.py; the scanline load and store around them are that tool's reading of
DirectXTexConvert.cpp:765-766 and :1634-1646); the host arithmetic of itwMipLevels and itwMipChainLayout; and everything
itwGenerateMipChain and itwCompressImageMipped refuse before any device work."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _mipgen as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _pins():
    with open(os.path.join(GOLD, "mipgen_ref_sha256.json")) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "mipgen_ref.npz")))


@pytest.mark.parametrize("name", sorted(_pins()))
def test_the_model_is_the_reference_filter(gold, name):
    e = _pins()[name]
    w, h = e["width"], e["height"]
    assert (e["filter"] == "box") == (M.is_pow2(w) and M.is_pow2(h))
    assert e["filter"] != "box" or h >= w, "wide power-of-two chains are not pinned: the reference reads stale storage there"
    base = M.seeded_half_image(h, w, e["seed"])
    assert hashlib.sha256(base.tobytes()).hexdigest() == e["input_sha256"], "the seeded input is not the recorded one"
    chain = M.chain(base)
    assert len(chain) == M.levels_of(w, h) and chain[-1].shape[:2] == (1, 1)
    assert hashlib.sha256(b"".join(l.tobytes() for l in chain[1:])).hexdigest() == e["levels_sha256"]
    if e["stored"]:
        assert np.array_equal(gold[name + "_in"], base)
        for i, lv in enumerate(chain[1:], 1):
            assert np.array_equal(gold[f"{name}_l{i}"], lv), (name, i)


def test_the_filter_tables_are_the_reference_tables(gold):
    names = [k for k in gold if k.startswith("filter_")]
    assert len(names) >= 10
    for k in names:
        source, dest = (int(v) for v in k.split("_")[1:])
        u0, w0, u1, w1 = M.linear_filter(source, dest)
        ref = gold[k]
        assert np.array_equal(ref[0], u0) and np.array_equal(ref[2], u1), k
        assert np.array_equal(ref[1].astype(np.float32).view(np.uint32), w0.view(np.uint32)), k
        assert np.array_equal(ref[3].astype(np.float32).view(np.uint32), w1.view(np.uint32)), k


def test_rgba8_box_is_the_integer_rule():
    rng = np.random.default_rng(5)
    for h, w in ((2, 2), (16, 8), (1, 8), (8, 1), (64, 64)):
        img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        assert np.array_equal(M.box_level(img), M.box_level_rgba8_integer(img))
    edge = np.array([[[0, 255, 255, 1], [0, 255, 255, 0]], [[0, 255, 254, 0], [0, 255, 255, 0]]], dtype=np.uint8)
    assert M.box_level(edge).tolist() == [[[0, 255, 255, 0]]]


def test_a_nan_stores_one_pattern_and_the_clamp_holds():
    v = np.array([np.nan, 70000.0, -70000.0, 65504.0, 65520.0, -0.0], dtype=np.float32)
    assert M.store_rgba16f(v).tolist() == [0x7E00, 0x7BFF, 0xFBFF, 0x7BFF, 0x7BFF, 0x8000]
    four = np.full((2, 2, 4), 0x7BFF, dtype=np.uint16)
    assert (M.box_level(four) == 0x7BFF).all()


def test_mip_levels_and_layout_against_the_model(itw):
    L = itw.lib()
    for w in range(1, 71):
        for h in range(1, 71):
            assert L.itwMipLevels(w, h) == M.levels_of(w, h), (w, h)
    for w, h in ((4096, 4096), (16384, 1), (1, 16384), (4000, 3000), (65535, 65536), (2 ** 28 - 1, 3), (2 ** 30, 2 ** 30)):
        assert L.itwMipLevels(w, h) == M.levels_of(w, h), (w, h)
    for w, h in ((0, 4), (4, 0), (-1, 4), (4, -7), (0, 0)):
        assert L.itwMipLevels(w, h) == 0
    S = itw.RgbaSurface
    base_ptr = 0x10000
    for w in range(1, 71):
        for h in (1, 2, 3, 7, 16, 33, 64, 70, w):
            full = M.levels_of(w, h)
            for px, items, levels in ((4, 1, 0), (8, 6, 0), (4, 3, 2), (8, 2, full), (4, 2, 1)):
                if levels > full:
                    continue
                n = levels or full
                out = (S * (items * n))()
                need = L.itwMipChainLayout(w, h, items, levels, px, base_ptr, C.cast(out, C.c_void_p))
                assert need == L.itwMipChainLayout(w, h, items, levels, px, None, None)
                at = 0
                for i in range(items):                       # DDS order: item-major, then level
                    for l in range(n):
                        lw, lh = M.level_size(w, h, l)
                        s = out[i * n + l]
                        assert (s.ptr, s.width, s.height, s.stride) == (base_ptr + at, lw, lh, lw * px), (w, h, px, i, l)
                        at += lw * lh * px
                assert need == at
    assert L.itwMipChainLayout(4096, 4096, 1, 0, 8, None, None) == sum((4096 >> l) ** 2 * 8 for l in range(13))
    assert L.itwMipChainLayout(2 ** 20, 2 ** 14, 2, 3, 4, None, None) == 2 * 4 * (2 ** 34 + 2 ** 32 + 2 ** 30)      # beyond 32 bits
    assert L.itwMipChainLayout(8, 8, 0, 0, 4, None, None) == 0
    for args in ((0, 8, 1, 0, 4), (8, 0, 1, 0, 4), (8, 8, -1, 0, 4), (8, 8, 1, -1, 4), (8, 8, 1, 5, 4), (8, 8, 1, 0, 3), (8, 8, 1, 0, 16), (2 ** 29, 1, 1, 1, 8)):
        assert L.itwMipChainLayout(*args, None, None) == -1, args
    size, entries = itw.mip_chain_layout(5, 3, items=2, pixel_size=8)
    assert size == 2 * 8 * (15 + 2 + 1) and [e[1:3] for e in entries] == [(5, 3), (2, 1), (1, 1)] * 2
    with pytest.raises(ValueError):
        itw.mip_chain_layout(8, 8, levels=9)


def test_generate_noops_return_zero_and_write_nothing(itw):
    L = itw.lib()
    S = itw.RgbaSurface
    img = np.full((8, 8, 4), 0xA5, np.uint8)
    lvl = np.full((4, 4, 4), 0x5A, np.uint8)
    arr = C.cast((S * 2)(S(img.ctypes.data, 8, 8, 32), S(lvl.ctypes.data, 4, 4, 16)), C.c_void_p)
    assert L.itwGenerateMipChain(arr, 0, 2, 4, 0) == 0
    assert L.itwGenerateMipChain(None, 0, 2, 4, 0) == 0
    assert L.itwGenerateMipChain(arr, 1, 1, 4, 0) == 0
    assert L.itwGenerateMipChain(arr, 1, 0, 4, 1) == 0
    assert L.itwGenerateMipChain(None, 3, 1, 8, 0) == 0
    assert (img == 0xA5).all() and (lvl == 0x5A).all()


def test_bad_mip_calls_return_before_any_device_use():
    """Fresh interpreter: the error mode is process-wide.  Every refusal leaves a message and writes nothing."""
    code = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
import itw_amd
L = itw_amd.lib()
S = itw_amd.RgbaSurface
itw_amd.set_error_mode(itw_amd.ON_ERROR_RETURN)
store = np.full(8 * 8 * 8 * 2, 0x11, np.uint8)
p = store.ctypes.data
assert p %% 8 == 0
def arr(*s):
    return C.cast((S * len(s))(*s), C.c_void_p)
def chain(px, w=8, h=8, levels=4, items=1, at=p):
    out = (S * (items * levels))()
    assert L.itwMipChainLayout(w, h, items, levels, px, at, C.cast(out, C.c_void_p)) > 0
    return out
n = 0
def refused(what, images, items, levels, px, flags):
    global n
    L.itwClearError()
    assert L.itwGenerateMipChain(images, items, levels, px, flags) == -1, what
    assert itw_amd.last_error(), what
    n += 1
good = chain(4)
refused("null images", None, 1, 4, 4, 0)
refused("pixel_size 3", C.cast(good, C.c_void_p), 1, 4, 3, 0)
refused("pixel_size 16", C.cast(good, C.c_void_p), 1, 4, 16, 0)
refused("unknown flag", C.cast(good, C.c_void_p), 1, 4, 4, 2)
refused("unknown high flag", C.cast(good, C.c_void_p), 1, 4, 4, 0x80000001)
refused("items < 0", C.cast(good, C.c_void_p), -1, 4, 4, 0)
c = chain(4); c[2].ptr = None
refused("null texels", C.cast(c, C.c_void_p), 1, 4, 4, 0)
c = chain(4); c[1].width = 3
refused("a level of the wrong width", C.cast(c, C.c_void_p), 1, 4, 4, 0)
c = chain(4); c[3].height = 2
refused("a level of the wrong height", C.cast(c, C.c_void_p), 1, 4, 4, 0)
c = chain(4, items=2, levels=2); c[2].width = 4; c[2].height = 4; c[3].width = 2; c[3].height = 2
refused("bases of different sizes", C.cast(c, C.c_void_p), 2, 2, 4, 0)
c = chain(4, levels=4)
five = (S * 5)(*c, S(p, 1, 1, 4))
refused("levels above the full chain", C.cast(five, C.c_void_p), 1, 5, 4, 0)
c = chain(4); c[0].width = 0
refused("a base of width 0", C.cast(c, C.c_void_p), 1, 4, 4, 0)
c = chain(4); c[1].stride = 12
refused("stride below the row", C.cast(c, C.c_void_p), 1, 4, 4, 0)
c = chain(8); c[1].stride = 24
refused("stride below the row (RGBA16F)", C.cast(c, C.c_void_p), 1, 4, 8, 0)
c = chain(4); c[1].ptr += 2
refused("misaligned texels", C.cast(c, C.c_void_p), 1, 4, 4, 0)
c = chain(8); c[0].ptr += 4
refused("misaligned texels (RGBA16F)", C.cast(c, C.c_void_p), 1, 4, 8, 0)
c = chain(8); c[0].stride = 68
refused("misaligned stride (RGBA16F)", C.cast(c, C.c_void_p), 1, 4, 8, 0)
many = (S * (65536 * 2))()                                  # more items than one launch covers: refused before any image but the first is read
many[0] = S(p, 8, 8, 32)
refused("65 536 items", C.cast(many, C.c_void_p), 65536, 2, 4, 0)
tall = (S * 2)(S(p, 1, 524282, 4), S(p, 1, 262141, 4))      # (never dereferenced: the size is refused first)
refused("more rows than one launch covers", C.cast(tall, C.c_void_p), 1, 2, 4, 0)
print("generate refused", n)

out = np.zeros(4096, np.uint8)
img = np.zeros((8, 8, 4), np.uint8)
small = np.zeros((4, 4, 4), np.uint8)
b8 = S(img.ctypes.data, 8, 8, 32)
bc7 = itw_amd.bc7_profile("ultrafast")
s7 = C.cast(C.byref(bc7), C.c_void_p)
etc0 = itw_amd.EtcSettings(0)
m = 0
def refused2(what, bases, items, levels, ops, target, fmt, settings):
    global m
    L.itwClearError()
    assert L.itwCompressImageMipped(bases, items, levels, ops, target, fmt, settings, None, None) is False, what
    assert itw_amd.last_error(), what
    m += 1
t = out.ctypes.data
refused2("unknown ops bit", arr(b8), 1, 0, 8, t, 71, None)
refused2("null bases", None, 1, 0, 0, t, 71, None)
refused2("no items", arr(b8), 0, 0, 0, t, 71, None)
refused2("negative items", arr(b8), -2, 0, 0, t, 71, None)
refused2("null target", arr(b8), 1, 0, 0, None, 71, None)
refused2("null texels", arr(S(None, 8, 8, 32)), 1, 0, 0, t, 71, None)
refused2("unknown format", arr(b8), 1, 0, 0, t, 0, None)
refused2("null BC7 settings", arr(b8), 1, 0, 0, t, 98, None)
refused2("null BC6H settings", arr(b8), 1, 0, 0, t, 95, None)
refused2("null ETC1 settings", arr(b8), 1, 0, 0, t, itw_amd.DXGI_FORMAT["etc1"], None)
refused2("ETC1 threshold 0", arr(b8), 1, 0, 0, t, itw_amd.DXGI_FORMAT["etc1"], C.cast(C.byref(etc0), C.c_void_p))
refused2("width 0", arr(S(img.ctypes.data, 0, 8, 32)), 1, 0, 0, t, 71, None)
refused2("stride below the row", arr(S(img.ctypes.data, 8, 8, 28)), 1, 0, 0, t, 98, s7)
refused2("levels above the full chain", arr(b8), 1, 5, 0, t, 98, s7)
refused2("negative levels", arr(b8), 1, -1, 0, t, 98, s7)
refused2("bases of different sizes", arr(b8, S(small.ctypes.data, 4, 4, 16)), 2, 0, 0, t, 98, s7)
refused2("misaligned texels", arr(S(img.ctypes.data + 1, 4, 4, 32)), 1, 0, 0, t, 98, s7)
refused2("more rows than one launch covers", arr(S(p, 1, 524282, 4)), 1, 2, 0, t, 71, None)
assert not out.any() and (store == 0x11).all()
print("mipped refused", m)
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.split("\n")[:2] == ["generate refused 19", "mipped refused 18"]
