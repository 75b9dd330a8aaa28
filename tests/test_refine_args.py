"""The argument checks of itwCompressImageRefined and the layout of itw_refine_stats (include/itw_dispatch.h): host-only, no GPU needed.

A bad call fails through the library's error mode BEFORE any device work: under ITW_ON_ERROR_RETURN it returns false with a message,
on a box without a GPU as on one with it."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bad_refined_calls_return_false_before_any_device_use():
    """Run in a fresh interpreter: the error mode is process-wide."""
    code = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
import itw_amd
L = itw_amd.lib()
itw_amd.set_error_mode(itw_amd.ON_ERROR_RETURN)
img = np.zeros((8, 8, 4), dtype=np.uint8)
out = np.zeros(4096, dtype=np.uint8)
raw = np.zeros(128, dtype=np.uint64)                     # 8-byte aligned room for the stats
a, b = itw_amd.bc7_profile("veryfast"), itw_amd.bc7_profile("slow")
A, B, S, SZ = C.addressof(a), C.addressof(b), raw.ctypes.data, C.sizeof(itw_amd.RefineStats)
def surf(w=8, h=8, stride=32, ptr=img.ctypes.data):
    return itw_amd.RgbaSurface(ptr, w, h, stride)
# (surface, format, first, refine, mask, stats, stats_bytes)
cases = {
    "format 71": (surf(), 71, A, B, 7, S, SZ),
    "null first settings": (surf(), 98, None, B, 7, S, SZ),
    "null refine settings": (surf(), 95, A, None, 7, S, SZ),
    "width 6": (surf(w=6), 98, A, B, 7, S, SZ),
    "height 0": (surf(h=0), 98, A, B, 7, S, SZ),
    "stride below the row": (surf(stride=31), 98, A, B, 7, S, SZ),
    "stride below a half-float row": (surf(stride=32), 95, A, B, 7, S, SZ),
    "mask 0": (surf(), 98, A, B, 0, S, SZ),
    "mask 16": (surf(), 98, A, B, 16, S, SZ),
    "stats_bytes one field short": (surf(), 98, A, B, 7, S, SZ - 8),
    "stats_bytes 0": (surf(), 98, A, B, 7, S, 0),
    "misaligned stats": (surf(), 98, A, B, 7, S + 4, SZ),
    "null stats": (surf(), 98, A, B, 7, None, SZ),
    "null texels": (surf(ptr=None), 98, A, B, 7, S, SZ),
}
for name, (s, fmt, first, refine, mask, stats, size) in cases.items():
    L.itwClearError()
    ok = L.itwCompressImageRefined(C.byref(s), out.ctypes.data, fmt, first, refine, mask, 100, stats, size, None, None)
    err = itw_amd.last_error()
    assert ok is False and err and "itwCompressImageRefined" in err, (name, ok, err)
L.itwClearError()
assert L.itwCompressImageRefined(None, out.ctypes.data, 98, A, B, 7, 100, S, SZ, None, None) is False and itw_amd.last_error()
L.itwClearError()
assert L.itwCompressImageRefined(C.byref(surf()), None, 98, A, B, 7, 100, S, SZ, None, None) is False and itw_amd.last_error()
L.itwClearError()
assert L.itwCompressImageRefined(C.byref(surf()), out.ctypes.data, 98, A, B, 7, 100, S, SZ, raw.ctypes.data + 68, None) is False and itw_amd.last_error()
assert not raw.any() and not out.any()
print("rejected", len(cases))
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "rejected 14"


def test_refine_stats_layout(itw, tmp_path):
    """sizeof(itw_refine_stats) is 56, and the binding's layout is the header's."""
    fields = ("blocks", "listed", "replaced", "sse_first", "sse_final", "worst_first", "worst_final")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "itw_dispatch.h"\n'
                   'int main(void) { printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(itw_refine_stats), '
                   + ", ".join(f"offsetof(itw_refine_stats, {f})" for f in fields) + "); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = itw.RefineStats
    assert [name for name, _ in S._fields_] == list(fields)
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert got[0] == 56 and got[1:] == [8 * k for k in range(7)]
