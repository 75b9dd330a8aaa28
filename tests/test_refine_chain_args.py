"""The argument checks of itwCompressImageChainRefined / itwCompressImageChainRefinedTo and the values of itwChainPsnrToTotalSse
(include/itw_dispatch.h): host-only, no GPU needed.

A bad call fails through the library's error mode BEFORE any device work: under ITW_ON_ERROR_RETURN it returns false with a message, on a
box without a GPU as on one with it.  Everything itwCompressImageChainEx and itwCompressImageRefined[To] refuse, a summed block count
above ITW_MEASURE_MAX_BLOCKS and a misaligned image_stats."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRELUDE = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
import itw_amd
L = itw_amd.lib()
img = np.zeros((8, 8, 4), dtype=np.uint8)
out = np.zeros(4096, dtype=np.uint8)
raw = np.zeros(256, dtype=np.uint64)                     # 8-byte aligned room for the stats, the per-image stats and a block map
a, b = itw_amd.bc7_profile("veryfast"), itw_amd.bc7_profile("slow")
pol = itw_amd.RefinePolicy(3, 2 ** 64 - 1)
A, B, P, PZ, S = C.addressof(a), C.addressof(b), C.addressof(pol), C.sizeof(pol), raw.ctypes.data
IS, BM = S + 512, S + 1024
SZ = {"budget": C.sizeof(itw_amd.RefineStats), "to": C.sizeof(itw_amd.RefineTargetStats)}
def surf(w=8, h=8, stride=32, ptr=img.ctypes.data):
    return itw_amd.RgbaSurface(ptr, w, h, stride)
def chain(*surfs):
    return (itw_amd.RgbaSurface * len(surfs))(*surfs)
two = chain(surf(), surf(w=3, h=5))
# (images, count, target, format, first, refine, mask, policy, policy_bytes, stats, stats_bytes delta, image_stats, block_sse)
def case(images=two, count=2, target=out.ctypes.data, fmt=98, first=A, refine=B, mask=7, policy=P, pz=PZ, stats=S, dsz=0, per=IS, bmap=BM):
    return (images, count, target, fmt, first, refine, mask, policy, pz, stats, dsz, per, bmap)
both = {
    "count 0": case(count=0),
    "count -1": case(count=-1),
    "null images": case(images=None),
    "null target": case(target=None),
    "null texels": case(images=chain(surf(), surf(ptr=None))),
    "null first settings": case(first=None),
    "null refine settings": case(fmt=95, refine=None),
    "null stats": case(stats=None),
    "width 0": case(images=chain(surf(), surf(w=0))),
    "height 0": case(images=chain(surf(h=0), surf())),
    "stride below the row": case(images=chain(surf(), surf(stride=31))),
    "stride below a half-float row": case(fmt=95),
    "format 71": case(fmt=71),
    "format 77": case(fmt=77),
    "format 80": case(fmt=80),
    "format 83": case(fmt=83),
    "mask 0": case(mask=0),
    "mask 16": case(mask=16),
    "stats_bytes one field short": case(dsz=-8),
    "stats_bytes one field long": case(dsz=8),
    "misaligned stats": case(stats=S + 4),
    "misaligned image_stats": case(per=IS + 4),
    "misaligned block_sse": case(bmap=BM + 4),
    "too many blocks": case(images=chain(surf(w=16384, h=16388, stride=65536), surf(w=16384, h=16388, stride=65536))),
}
to_only = {
    "null policy": case(policy=None),
    "policy_bytes one field short": case(pz=PZ - 8),
    "policy_bytes 0": case(pz=0),
}
def call(entry, c):
    images, count, target, fmt, first, refine, mask, policy, pz, stats, dsz, per, bmap = c
    if entry == "budget":
        return L.itwCompressImageChainRefined(images, count, target, fmt, first, refine, mask, 1000, stats, SZ[entry] + dsz, per, bmap, None)
    return L.itwCompressImageChainRefinedTo(images, count, target, fmt, first, refine, mask, policy, pz, stats, SZ[entry] + dsz, per, bmap, None)
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")


def test_bad_calls_return_false_before_any_device_use():
    """Run in a fresh interpreter: the error mode is process-wide.  The limit case: two 16384 x 16388 images are 2 x 16 781 312 =
    33 562 624 blocks, each below ITW_MEASURE_MAX_BLOCKS = 33 554 432 and their sum above it."""
    code = PRELUDE + r"""
itw_amd.set_error_mode(itw_amd.ON_ERROR_RETURN)
n = 0
for entry, cases in (("budget", both), ("to", {**both, **to_only})):
    for name, c in cases.items():
        L.itwClearError()
        ok = call(entry, c)
        err = itw_amd.last_error()
        assert ok is False and err and "itwCompressImageChain" in err, (entry, name, ok, err)
        n += 1
L.itwClearError()
assert call("budget", both["too many blocks"]) is False and "33554432" in itw_amd.last_error()
assert not raw.any() and not out.any()
print("rejected", n)
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "rejected 51"


def test_the_symbols_are_exported_and_declared(itw):
    L = itw.lib()
    with open(os.path.join(ROOT, "include", "itw_dispatch.h")) as f:
        header = f.read()
    for name in ("itwCompressImageChainRefined", "itwCompressImageChainRefinedTo", "itwChainPsnrToTotalSse"):
        assert name in itw.EXPORTED_SYMBOLS and getattr(L, name) and name + "(" in header
    for name in ("compress_chain_refined", "compress_chain_refined_to", "chain_psnr_to_total_sse"):
        assert callable(getattr(itw, name))


def _chain(itw, sizes):
    return (itw.RgbaSurface * len(sizes))(*[itw.RgbaSurface(None, w, h, 0) for w, h in sizes])


def test_chain_psnr_to_total_sse_is_psnr_to_total_sse_over_all_texels(itw):
    L = itw.lib()
    sizes = [(132, 100), (66, 50), (33, 25), (16, 12), (8, 6), (4, 3), (2, 1), (1, 1), (7, 5), (3, 11)]
    texels = sum(w * h for w, h in sizes)
    arr = _chain(itw, sizes)
    for mask, n in ((7, 3), (15, 4), (1, 1), (10, 2)):
        for db in (0.0, 20.0, 33.3, 45.0, 60.0, 99.0, -10.0):
            want = math.floor(255.0 * 255.0 * (texels * n) / 10.0 ** (db / 10.0))
            assert abs(L.itwChainPsnrToTotalSse(C.cast(arr, C.c_void_p), len(sizes), 98, mask, db) - want) <= 1, (mask, db)
    assert L.itwChainPsnrToTotalSse(C.cast(arr, C.c_void_p), len(sizes), 98, 7, 30.0) == math.floor(65025.0 * texels * 3 / 1000.0)      # 10^3 is exact
    # one image: the single-image helper's value; a square image in four quarters: the whole image's value
    for db in (12.5, 30.0, 41.7):
        one = _chain(itw, [(68, 36)])
        assert L.itwChainPsnrToTotalSse(C.cast(one, C.c_void_p), 1, 99, 15, db) == L.itwPsnrToTotalSse(99, 68, 36, 15, db)
        four = _chain(itw, [(32, 32)] * 4)
        assert L.itwChainPsnrToTotalSse(C.cast(four, C.c_void_p), 4, 98, 7, db) == L.itwPsnrToTotalSse(98, 64, 64, 7, db)
    assert itw.chain_psnr_to_total_sse("bc7", [(h, w) for w, h in sizes], 30.0) == math.floor(65025.0 * texels * 3 / 1000.0)
    assert itw.chain_psnr_to_total_sse("bc7", [np.zeros((5, 3, 4), dtype=np.uint8)], 20.0, "rgba") == math.floor(65025.0 * 15 * 4 / 100.0)


def test_chain_psnr_to_total_sse_has_no_answer_where_psnr_to_total_sse_has_none(itw):
    L = itw.lib()
    U = 2 ** 64 - 1
    arr = _chain(itw, [(64, 64), (32, 32)])
    p = C.cast(arr, C.c_void_p)
    assert L.itwChainPsnrToTotalSse(p, 2, 98, 7, 40.0) == math.floor(65025.0 * 5120 * 3 / 10000.0)
    for fmt in (95, 96, 0, 1234):                                  # BC6H; no format
        assert L.itwChainPsnrToTotalSse(p, 2, fmt, 7, 40.0) == U
    for mask in (0, 16, 32):
        assert L.itwChainPsnrToTotalSse(p, 2, 98, mask, 40.0) == U
    for db in (math.nan, math.inf, -math.inf):
        assert L.itwChainPsnrToTotalSse(p, 2, 98, 7, db) == U
    for count in (0, -1):
        assert L.itwChainPsnrToTotalSse(p, count, 98, 7, 40.0) == U
    assert L.itwChainPsnrToTotalSse(None, 2, 98, 7, 40.0) == U
    for bad in ([(64, 64), (0, 32)], [(64, -4), (32, 32)]):
        assert L.itwChainPsnrToTotalSse(C.cast(_chain(itw, bad), C.c_void_p), 2, 98, 7, 40.0) == U
    assert L.itwChainPsnrToTotalSse(p, 2, 98, 7, -2000.0) == U     # beyond 64 bits
    assert L.itwChainPsnrToTotalSse(p, 2, 98, 7, 2000.0) == 0
