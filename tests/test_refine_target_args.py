"""The argument checks of itwCompressImageRefinedTo, the layout of its two structs and itwPsnrToTotalSse (include/itw_dispatch.h):
host-only, no GPU needed.

A bad call fails through the library's error mode BEFORE any device work: under ITW_ON_ERROR_RETURN it returns false with a message,
under ITW_ON_ERROR_ABORT the process prints the message and aborts, on a box without a GPU as on one with it."""
import ctypes as C
import math
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the five errors the entry adds, then itwCompressImageRefined's own, as (source, format, first, refine, mask, policy, policy_bytes, stats, stats_bytes)
PRELUDE = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
import itw_amd
L = itw_amd.lib()
img = np.zeros((8, 8, 4), dtype=np.uint8)
out = np.zeros(4096, dtype=np.uint8)
raw = np.zeros(128, dtype=np.uint64)                     # 8-byte aligned room for the stats
a, b = itw_amd.bc7_profile("veryfast"), itw_amd.bc7_profile("slow")
pol = itw_amd.RefinePolicy(3, 2 ** 64 - 1)
A, B, P, PZ, S, SZ = C.addressof(a), C.addressof(b), C.addressof(pol), C.sizeof(pol), raw.ctypes.data, C.sizeof(itw_amd.RefineTargetStats)
def surf(w=8, h=8, stride=32, ptr=img.ctypes.data):
    return itw_amd.RgbaSurface(ptr, w, h, stride)
new = {
    "null policy": (surf(), 98, A, B, 7, None, PZ, S, SZ),
    "policy_bytes one field short": (surf(), 98, A, B, 7, P, PZ - 8, S, SZ),
    "policy_bytes 0": (surf(), 98, A, B, 7, P, 0, S, SZ),
    "null stats": (surf(), 98, A, B, 7, P, PZ, None, SZ),
    "stats_bytes of itw_refine_stats": (surf(), 98, A, B, 7, P, PZ, S, C.sizeof(itw_amd.RefineStats)),
    "stats_bytes one field long": (surf(), 98, A, B, 7, P, PZ, S, SZ + 8),
    "misaligned stats": (surf(), 98, A, B, 7, P, PZ, S + 4, SZ),
}
old = {
    "format 71": (surf(), 71, A, B, 7, P, PZ, S, SZ),
    "null first settings": (surf(), 98, None, B, 7, P, PZ, S, SZ),
    "null refine settings": (surf(), 95, A, None, 7, P, PZ, S, SZ),
    "width 6": (surf(w=6), 98, A, B, 7, P, PZ, S, SZ),
    "height 0": (surf(h=0), 98, A, B, 7, P, PZ, S, SZ),
    "stride below the row": (surf(stride=31), 98, A, B, 7, P, PZ, S, SZ),
    "stride below a half-float row": (surf(stride=32), 95, A, B, 7, P, PZ, S, SZ),
    "mask 0": (surf(), 98, A, B, 0, P, PZ, S, SZ),
    "mask 16": (surf(), 98, A, B, 16, P, PZ, S, SZ),
    "null texels": (surf(ptr=None), 98, A, B, 7, P, PZ, S, SZ),
}
def call(case, target=out.ctypes.data, bmap=None):
    s, fmt, first, refine, mask, policy, pz, stats, sz = case
    return L.itwCompressImageRefinedTo(C.byref(s), target, fmt, first, refine, mask, policy, pz, stats, sz, bmap, None)
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")

NEW = ("null policy", "policy_bytes one field short", "policy_bytes 0", "null stats", "stats_bytes of itw_refine_stats", "stats_bytes one field long",
       "misaligned stats")


def test_bad_calls_return_false_before_any_device_use():
    """Run in a fresh interpreter: the error mode is process-wide."""
    code = PRELUDE + r"""
itw_amd.set_error_mode(itw_amd.ON_ERROR_RETURN)
for name, case in {**new, **old}.items():
    L.itwClearError()
    ok = call(case)
    err = itw_amd.last_error()
    assert ok is False and err and "itwCompressImageRefinedTo" in err, (name, ok, err)
L.itwClearError()
assert L.itwCompressImageRefinedTo(None, out.ctypes.data, 98, A, B, 7, P, PZ, S, SZ, None, None) is False and itw_amd.last_error()
L.itwClearError()
assert call(new["misaligned stats"][:7] + (S, SZ), target=None) is False and itw_amd.last_error()
L.itwClearError()
assert call(new["misaligned stats"][:7] + (S, SZ), bmap=raw.ctypes.data + 68) is False and itw_amd.last_error()
assert not raw.any() and not out.any()
print("rejected", len(new), len(old))
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "rejected 7 10"


@pytest.mark.parametrize("name", NEW)
def test_bad_calls_abort_with_the_message_in_abort_mode(name):
    """The default mode: the diagnostic on stderr, then abort() -- a child process each, which ends before it touches a device."""
    code = PRELUDE + r"""
itw_amd.set_error_mode(itw_amd.ON_ERROR_ABORT)
sys.stdout.write("calling\n"); sys.stdout.flush()
call(new[%r])
print("returned")
""" % name
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == -signal.SIGABRT, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert r.stdout.strip() == "calling" and "itwCompressImageRefinedTo" in r.stderr


def test_structs_layout(itw, tmp_path):
    """sizeof and every offset of itw_refine_policy and itw_refine_target_stats: the binding's layout is the header's."""
    fields = {"itw_refine_policy": ("max_listed", "target_total_sse"), "itw_refine_target_stats": ("total", "rounds", "target_met", "budget", "listed")}
    body = "".join('printf("%zu' + " %zu" * len(f) + '\\n", sizeof(' + t + "), " + ", ".join(f"offsetof({t}, {x})" for x in f) + ");\n"
                   for t, f in fields.items())
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "itw_dispatch.h"\nint main(void) {\n' + body + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    for line, (t, f), S in zip(lines, fields.items(), (itw.RefinePolicy, itw.RefineTargetStats)):
        assert [name for name, _ in S._fields_] == list(f)
        assert [int(x) for x in line.split()] == [C.sizeof(S)] + [getattr(S, x).offset for x in f], t
    assert C.sizeof(itw.RefinePolicy) == 16 and C.sizeof(itw.RefineTargetStats) == 144
    assert [getattr(itw.RefineTargetStats, x).offset for x in fields["itw_refine_target_stats"]] == [0, 56, 60, 64, 104]


def test_the_symbols_are_exported(itw):
    L = itw.lib()
    for name in ("itwCompressImageRefinedTo", "itwPsnrToTotalSse"):
        assert name in itw.EXPORTED_SYMBOLS and getattr(L, name)


def _stats(itw, fmt, w, h, sse):
    s = itw.ErrorStats()
    s.dxgi_format, s.width, s.height = fmt, w, h
    s.blocks = ((w + 3) // 4) * ((h + 3) // 4)
    for c in range(4):
        s.sse[c] = sse[c]
    return s


@pytest.mark.parametrize("mask", [1, 6, 7, 8, 15])
@pytest.mark.parametrize("w,h", [(4, 4), (68, 36), (1024, 1024), (16384, 8192)])
def test_psnr_to_total_sse_inverts_stats_psnr(itw, w, h, mask):
    """S = the summed error of the selected channels; itwPsnrToTotalSse(itwStatsPsnr(S)) is S or S - 1.

    The helper floors 255^2 n / 10^(dB/10): in exact arithmetic that is S itself, and the two roundings of log10 and pow (a few 1e-16
    relative, far below 1 / S for any S an image of at most 2^25 blocks has: S < 2^44) can only leave the quotient a hair below S, where
    the floor gives S - 1, or a hair above, where it gives S.  Never S + 1 or more: a target from a PSNR is never looser than that PSNR."""
    L = itw.lib()
    rng = np.random.default_rng(w * 16 + mask)
    picked = [c for c in range(4) if mask >> c & 1]
    for fmt in (98, 99, 71, 77):
        for top in (1, 1000, w * h * 255 * 255):
            sse = [int(v) for v in rng.integers(1, top + 1, size=4)]
            total = sum(sse[c] for c in picked)
            db = L.itwStatsPsnr(C.byref(_stats(itw, fmt, w, h, sse)), mask)
            got = L.itwPsnrToTotalSse(fmt, w, h, mask, db)
            assert total - 1 <= got <= total, (fmt, w, h, mask, total, got, db)


def test_psnr_to_total_sse_is_the_floor_of_the_formula(itw):
    L = itw.lib()
    for w, h, mask, n in ((64, 64, 7, 3), (128, 72, 15, 4), (4, 4, 1, 1)):
        for db in (0.0, 20.0, 33.3, 45.0, 60.0, 99.0, -10.0):
            want = math.floor(255.0 * 255.0 * (w * h * n) / 10.0 ** (db / 10.0))
            assert abs(L.itwPsnrToTotalSse(98, w, h, mask, db) - want) <= 1, (w, h, mask, db)
    assert L.itwPsnrToTotalSse(98, 64, 64, 7, 30.0) == math.floor(65025.0 * 12288 / 1000.0)      # 10^3 is exact
    assert L.itwPsnrToTotalSse(81, 64, 64, 1, 20.0) == math.floor(254.0 * 254.0 * 4096 / 100.0)   # the SNORM pair's peak, as itwStatsPsnr


def test_psnr_to_total_sse_has_no_answer_where_stats_psnr_has_none(itw):
    L = itw.lib()
    U = 2 ** 64 - 1
    for fmt in (95, 96, 0, 1234):                                  # BC6H; no format
        assert L.itwPsnrToTotalSse(fmt, 64, 64, 7, 40.0) == U
    for mask in (0, 16, 32):                                       # no channel among the four
        assert L.itwPsnrToTotalSse(98, 64, 64, mask, 40.0) == U
    for db in (math.nan, math.inf, -math.inf):
        assert L.itwPsnrToTotalSse(98, 64, 64, 7, db) == U
    assert L.itwPsnrToTotalSse(98, 0, 64, 7, 40.0) == U and L.itwPsnrToTotalSse(98, 64, -4, 7, 40.0) == U
    assert L.itwPsnrToTotalSse(98, 64, 64, 7, -2000.0) == U        # beyond 64 bits
    assert L.itwPsnrToTotalSse(98, 64, 64, 7, 2000.0) == 0
