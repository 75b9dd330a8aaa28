"""itwChainBytes and the argument checks of itwCompressImageChain[Ex] (include/itw_dispatch.h): host-only, no GPU needed.

A bad call fails through the library's error mode BEFORE any device work: under ITW_ON_ERROR_RETURN it returns false with a message,
on a box without a GPU as on one with it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = (71, 72, 77, 78, 80, 83, 95, 96, 98, 99)


def _surfaces(itw, sizes):
    return (itw.RgbaSurface * len(sizes))(*[itw.RgbaSurface(None, w, h, 4 * w) for h, w in sizes])


@pytest.mark.parametrize("fmt", FORMATS)
def test_chain_bytes_is_the_sum_of_the_dds_level_sizes(itw, fmt):
    L = itw.lib()
    L.itwDdsLevelBytes.restype = C.c_size_t
    L.itwDdsLevelBytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    rng = np.random.default_rng(fmt)
    lists = [[(1, 1)], [(3, 2)], [(7, 5)], [(1, 1), (3, 2), (7, 5)]]
    lists += [[(int(h), int(w)) for h, w in rng.integers(1, 3000, size=(int(rng.integers(1, 70)), 2))] for _ in range(20)]
    for sizes in lists:
        arr = _surfaces(itw, sizes)
        want = sum(L.itwDdsLevelBytes(fmt, w, h) for h, w in sizes)
        assert L.itwChainBytes(C.cast(arr, C.c_void_p), len(sizes), fmt) == want, (fmt, sizes[:4])


def test_chain_bytes_of_a_mip_chain_and_the_binding(itw):
    levels = itw.mip_chain(np.zeros((1023, 517, 4), np.uint8))
    assert [lv.shape[:2] for lv in levels][:3] == [(1023, 517), (511, 258), (255, 129)] and levels[-1].shape[:2] == (1, 1)
    assert len(levels) == 10
    want = sum(((lv.shape[0] + 3) // 4) * ((lv.shape[1] + 3) // 4) for lv in levels)
    assert itw.chain_bytes("bc7", levels) == 16 * want
    assert itw.chain_bytes("bc1", levels) == 8 * want
    assert itw.chain_bytes("bc4", [(5, 7)]) == 8 * 4


def test_chain_bytes_rejects_bad_arguments(itw):
    L = itw.lib()
    ok = _surfaces(itw, [(4, 4)])
    assert L.itwChainBytes(None, 1, 71) == -1
    assert L.itwChainBytes(C.cast(ok, C.c_void_p), 0, 71) == -1
    assert L.itwChainBytes(C.cast(ok, C.c_void_p), 1, 0) == -1
    assert L.itwChainBytes(C.cast(ok, C.c_void_p), 1, 28) == -1          # R8G8B8A8: not a format this library encodes
    bad = _surfaces(itw, [(4, 4), (0, 4)])
    assert L.itwChainBytes(C.cast(bad, C.c_void_p), 2, 71) == -1


def test_bad_chain_calls_return_false_before_any_device_use():
    """Each bad call returns false with a message under ITW_ON_ERROR_RETURN.  Run in a fresh interpreter: the error mode is process-wide."""
    code = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
import itw_amd
L = itw_amd.lib()
itw_amd.set_error_mode(itw_amd.ON_ERROR_RETURN)
img = np.zeros((8, 8, 4), dtype=np.uint8)
out = np.zeros(4096, dtype=np.uint8)
def arr(*s):
    return C.cast((itw_amd.RgbaSurface * len(s))(*s), C.c_void_p)
good = itw_amd.RgbaSurface(img.ctypes.data, 8, 8, 32)
s7 = itw_amd.bc7_profile("basic")
cases = {
    "count 0": (arr(good), 0, 71, None),
    "null images": (None, 1, 71, None),
    "0-width image": (arr(good, itw_amd.RgbaSurface(img.ctypes.data, 0, 8, 32)), 2, 71, None),
    "0-height image": (arr(itw_amd.RgbaSurface(img.ctypes.data, 8, 0, 32)), 1, 98, C.cast(C.byref(s7), C.c_void_p)),
    "format 0": (arr(good), 1, 0, None),
    "BC7 with null settings": (arr(good), 1, 98, None),
    "BC6H with null settings": (arr(good), 1, 95, None),
    "null texels": (arr(itw_amd.RgbaSurface(None, 8, 8, 32)), 1, 71, None),
    "stride below the row": (arr(itw_amd.RgbaSurface(img.ctypes.data, 8, 8, 31)), 1, 71, None),
}
for name, (images, count, fmt, settings) in cases.items():
    itw_amd.lib().itwClearError()
    ok = L.itwCompressImageChainEx(images, count, out.ctypes.data, fmt, settings, None, None)
    err = itw_amd.last_error()
    assert ok is False and err, (name, ok, err)
    if name not in ("BC7 with null settings", "BC6H with null settings"):      # (a trampoline brings its own settings)
        itw_amd.lib().itwClearError()                                        # the trampoline variant checks the same arguments
        ok = L.itwCompressImageChain(images, count, out.ctypes.data, itw_amd.image_func("bc1"), fmt, None, None)
        assert ok is False and itw_amd.last_error(), ("trampoline", name, ok)
assert L.itwCompressImageChainEx(arr(good), 1, None, 71, None, None, None) is False and itw_amd.last_error()
print("rejected", len(cases))
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "rejected 9"
