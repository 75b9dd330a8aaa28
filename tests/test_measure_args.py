"""itwStatsPsnr, the layout of itw_error_stats and the argument checks of itwMeasureBlocks / itwMeasureChain (include/itw_decode.h):
host-only, no GPU needed.  A bad call returns -1 BEFORE any device work, on a box without a GPU as on one with it."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stats(itw, fmt, w, h, sse):
    s = itw.ErrorStats()
    s.dxgi_format, s.width, s.height = fmt, w, h
    s.blocks = ((w + 3) // 4) * ((h + 3) // 4)
    for c in range(4):
        s.sse[c] = sse[c]
    return s


@pytest.mark.parametrize("fmt", [71, 72, 77, 78, 80, 83, 98, 99])
@pytest.mark.parametrize("mask", [1, 2, 4, 8, 3, 7, 15, 9])
def test_stats_psnr_is_the_formula_in_float64(itw, fmt, mask):
    L = itw.lib()
    rng = np.random.default_rng(fmt * 16 + mask)
    for w, h in ((1, 1), (5, 3), (256, 256), (1023, 517), (16384, 16384)):
        top = w * h * 255 * 255                                  # the largest sum a channel can have
        sse = [int(v) for v in rng.integers(1, top + 1, size=4)]
        s = _stats(itw, fmt, w, h, sse)
        picked = [c for c in range(4) if mask >> c & 1]
        total = np.float64(sum(sse[c] for c in picked))
        want = 10.0 * np.log10(np.float64(255.0 * 255.0) * np.float64(w * h * len(picked)) / total)
        got = L.itwStatsPsnr(C.byref(s), mask)
        assert abs(got - float(want)) <= 1e-9, (fmt, mask, w, h, got, want)


def test_stats_psnr_edges(itw):
    L = itw.lib()
    zero = _stats(itw, 98, 64, 64, [0, 0, 0, 7])
    assert L.itwStatsPsnr(C.byref(zero), 7) == math.inf            # the selected channels' sum is 0
    assert math.isfinite(L.itwStatsPsnr(C.byref(zero), 15))
    assert math.isnan(L.itwStatsPsnr(C.byref(zero), 0))            # empty mask
    assert math.isnan(L.itwStatsPsnr(C.byref(zero), 16))           # no channel among the four
    for f in (95, 96):                                             # BC6H: codes are half-float bit patterns
        assert math.isnan(L.itwStatsPsnr(C.byref(_stats(itw, f, 64, 64, [1, 2, 3, 4])), 7))
        assert math.isnan(L.itwStatsPsnr(C.byref(_stats(itw, f, 64, 64, [0, 0, 0, 0])), 7))


def test_the_binding_wraps_psnr_and_mse(itw):
    s = _stats(itw, 83, 10, 6, [120, 60, 999, 5])
    assert s.mse("rg") == (120 + 60) / (10 * 6 * 2.0) and s.mse() == s.mse("rg") and s.mse([2]) == 999 / 60.0
    assert abs(s.psnr("r") - 10 * math.log10(255.0 ** 2 * 60 / 120)) <= 1e-9
    assert s.psnr() == s.psnr((0, 1))
    with pytest.raises(ValueError):
        _stats(itw, 95, 4, 4, [1, 1, 1, 1]).psnr("rgb")
    assert _stats(itw, 95, 4, 4, [1, 2, 3, 4]).mse() == 6 / 48.0     # sums and means of codes stay available


def test_error_stats_layout_is_the_headers(itw, tmp_path):
    """The binding's struct is the header's (C, not C++: the header is a plain C header)."""
    src = tmp_path / "layout.c"
    fields = ("dxgi_format", "width", "height", "reserved_blocks", "blocks", "sse", "max_abs", "worst_block_sse", "worst_block", "mode_hist")
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "itw_decode.h"\n'
                   'int main(void) { printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(itw_error_stats)'
                   + "".join(f", offsetof(itw_error_stats, {f})" for f in fields) + "); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = itw.ErrorStats
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert C.sizeof(S) == 216


def test_bad_measure_calls_return_minus_one_before_any_device_use():
    """Each bad argument returns -1 and leaves no error behind (nothing was attempted).  A fresh interpreter, as for the chain's checks."""
    code = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
import itw_amd
L = itw_amd.lib()
itw_amd.set_error_mode(itw_amd.ON_ERROR_RETURN)
S = itw_amd.RgbaSurface
n = C.sizeof(itw_amd.ErrorStats)
img = np.zeros((8, 8, 4), dtype=np.uint8)
hdr = np.zeros((8, 8, 4), dtype=np.uint16)
blk = np.zeros(4096, dtype=np.uint8)
st = (itw_amd.ErrorStats * 4)()
stp = C.addressof(st)
bmap = np.zeros(16, dtype=np.uint64)
good = S(img.ctypes.data, 8, 8, 32)
cases = {
    "format 0": (0, blk.ctypes.data, good, stp, n, None),
    "format 28": (28, blk.ctypes.data, good, stp, n, None),
    "null blocks": (98, None, good, stp, n, None),
    "null source": (98, blk.ctypes.data, None, stp, n, None),
    "null texels": (98, blk.ctypes.data, S(None, 8, 8, 32), stp, n, None),
    "null stats": (98, blk.ctypes.data, good, None, n, None),
    "width 0": (71, blk.ctypes.data, S(img.ctypes.data, 0, 8, 32), stp, n, None),
    "height 0": (80, blk.ctypes.data, S(img.ctypes.data, 8, 0, 32), stp, n, None),
    "negative width": (77, blk.ctypes.data, S(img.ctypes.data, -4, 8, 32), stp, n, None),
    "stride below the row": (98, blk.ctypes.data, S(img.ctypes.data, 8, 8, 31), stp, n, None),
    "half stride below the row": (95, blk.ctypes.data, S(hdr.ctypes.data, 8, 8, 63), stp, n, None),
    "stats_bytes short": (98, blk.ctypes.data, good, stp, n - 8, None),
    "stats_bytes long": (98, blk.ctypes.data, good, stp, n + 8, None),
    "stats_bytes 0": (98, blk.ctypes.data, good, stp, 0, None),
    "too many blocks": (71, blk.ctypes.data, S(img.ctypes.data, 32768, 16388, 32768 * 4), stp, n, None),
}
for name, (fmt, b, s, stats, nbytes, m) in cases.items():
    L.itwClearError()
    rc = L.itwMeasureBlocks(fmt, b, C.byref(s) if s is not None else None, stats, nbytes, m)
    assert rc == -1 and itw_amd.last_error() is None, (name, rc, itw_amd.last_error())
def arr(*s):
    return C.cast((S * len(s))(*s), C.c_void_p)
chain = {
    "count 0": (arr(good), 0, blk.ctypes.data, 71, stp, n),
    "null images": (None, 1, blk.ctypes.data, 71, stp, n),
    "null blocks": (arr(good), 1, None, 71, stp, n),
    "null stats": (arr(good), 1, blk.ctypes.data, 71, None, n),
    "format 0": (arr(good), 1, blk.ctypes.data, 0, stp, n),
    "second image 0 wide": (arr(good, S(img.ctypes.data, 0, 8, 32)), 2, blk.ctypes.data, 98, stp, n),
    "second image null": (arr(good, S(None, 4, 4, 16)), 2, blk.ctypes.data, 98, stp, n),
    "stride below the row": (arr(S(img.ctypes.data, 8, 8, 31)), 1, blk.ctypes.data, 71, stp, n),
    "stats_bytes": (arr(good), 1, blk.ctypes.data, 71, stp, n + 1),
}
for name, a in chain.items():
    L.itwClearError()
    rc = L.itwMeasureChain(*a)
    assert rc == -1 and itw_amd.last_error() is None, ("chain", name, rc, itw_amd.last_error())
# the limit admits 16384^2 (2^24 blocks): with good arguments the call gets as far as the device
if not itw_amd.available():
    rc = L.itwMeasureBlocks(71, blk.ctypes.data, C.byref(good), stp, n, bmap.ctypes.data)
    assert rc == -1 and itw_amd.last_error(), "a good call without a GPU fails through the error mode, with a message"
print("rejected", len(cases), len(chain))
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "rejected 15 9"


def test_the_block_limit_admits_16384_squared():
    hdr = open(os.path.join(ROOT, "include", "itw_decode.h")).read()
    import re
    limit = int(re.search(r"#define\s+ITW_MEASURE_MAX_BLOCKS\s+(\d+)", hdr).group(1))
    assert limit >= (16384 // 4) ** 2
    assert (64 * 0xFFFF ** 2) * limit <= 2 ** 64                 # BC6H's largest block sum and the index share one 64-bit key
