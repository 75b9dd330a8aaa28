"""What the normal-map entry points refuse before any device work, and the host arithmetic of itwCubeCrossFaces (include/itw_dispatch.h,
include/itw_bc45.h): host-only, no GPU needed.  Also here: the numpy checker of tests/_normal_prep.py hashes to the recorded output of
the reference's own normalise loop over all 2^24 RGB triples (tests/golden/normal_prep_sha256.json)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _normal_prep as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_checker_is_the_reference_loop_over_all_triples():
    with open(os.path.join(ROOT, "tests", "golden", "normal_prep_sha256.json")) as f:
        pin = json.load(f)["normalize_rgb8_all_triples"]
    img = N.all_triples()
    out = N.prepare_rgba8(img, N.NORMALIZE)
    assert hashlib.sha256(np.ascontiguousarray(out[..., :3]).tobytes()).hexdigest() == pin
    assert np.array_equal(out[..., 3], img[..., 3])
    assert out.reshape(-1, 4)[(128 << 16) | (128 << 8) | 128, :3].tolist() == [128, 128, 255]        # the zero vector: the default normal


def _arr(itw, *s):
    return C.cast((itw.RgbaSurface * len(s))(*s), C.c_void_p)


def test_prepare_refuses_bad_calls_and_accepts_the_empty_ones(itw):
    L = itw.lib()
    S = itw.RgbaSurface
    img = np.zeros((8, 8, 4), np.uint16)                     # 512 bytes, 8-byte aligned by numpy: room for either texel size
    p = img.ctypes.data
    assert p % 8 == 0
    before = img.copy()
    good = S(p, 8, 8, 32)
    call = L.itwPrepareNormalMapChain
    assert call(_arr(itw, good), 0, 4, 7) == 0               # nothing to do
    assert call(None, 0, 4, 7) == 0
    assert call(_arr(itw, good), 1, 4, 0) == 0
    assert call(_arr(itw, S(p, 8, 8, 64)), 1, 8, 0) == 0
    refused = {
        "null images": (None, 1, 4, 4),
        "null texels": (_arr(itw, S(None, 8, 8, 32)), 1, 4, 4),
        "null texels in the second image": (_arr(itw, good, S(None, 8, 8, 32)), 2, 4, 4),
        "count < 0": (_arr(itw, good), -1, 4, 4),
        "pixel_size 3": (_arr(itw, good), 1, 3, 4),
        "pixel_size 16": (_arr(itw, good), 1, 16, 4),
        "pixel_size 0": (_arr(itw, good), 1, 0, 4),
        "unknown ops bit": (_arr(itw, good), 1, 4, 8),
        "unknown high ops bit": (_arr(itw, good), 1, 4, 0x80000001),
        "width 0": (_arr(itw, S(p, 0, 8, 32)), 1, 4, 4),
        "height 0": (_arr(itw, S(p, 8, 0, 32)), 1, 4, 4),
        "negative width": (_arr(itw, S(p, -4, 8, 32)), 1, 4, 4),
        "stride below the row (RGBA8)": (_arr(itw, S(p, 8, 8, 28)), 1, 4, 4),
        "stride below the row (RGBA16F)": (_arr(itw, S(p, 8, 8, 56)), 1, 8, 4),
        "negative stride": (_arr(itw, S(p, 8, 8, -32)), 1, 4, 4),
        "misaligned pointer (RGBA8)": (_arr(itw, S(p + 2, 4, 4, 32)), 1, 4, 4),
        "misaligned pointer (RGBA16F)": (_arr(itw, S(p + 4, 4, 4, 64)), 1, 8, 4),
        "misaligned stride (RGBA8)": (_arr(itw, S(p, 4, 4, 18)), 1, 4, 4),
        "misaligned stride (RGBA16F)": (_arr(itw, S(p, 4, 4, 36)), 1, 8, 4),
    }
    for name, (images, count, px, ops) in refused.items():
        assert call(images, count, px, ops) == -1, name
        if ops == 4:                                          # the same refusals come before the "nothing to do" of ops == 0
            assert call(images, count, px, 0) == -1, name + " (ops 0)"
    assert np.array_equal(img, before)


def test_bad_normal_map_encodes_return_before_any_device_use():
    """Unknown ops bits fail through the error mode (fresh interpreter: the mode is process-wide); the chain call's own refusals stay."""
    code = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
import itw_amd
L = itw_amd.lib()
itw_amd.set_error_mode(itw_amd.ON_ERROR_RETURN)
img = np.zeros((8, 8, 4), dtype=np.uint8)
out = np.zeros(4096, dtype=np.uint8)
good = itw_amd.RgbaSurface(img.ctypes.data, 8, 8, 32)
arr = C.cast((itw_amd.RgbaSurface * 1)(good), C.c_void_p)
n = 0
for ops in (8, 16, 0x107, 0x80000000):
    L.itwClearError()
    assert L.itwCompressNormalMapChain(arr, 1, out.ctypes.data, 83, None, ops, None, None) is False and "ops" in itw_amd.last_error(), ops
    L.itwClearError()
    L.itwCompressNormalMapBC5(C.byref(good), out.ctypes.data, ops)
    assert "ops" in (itw_amd.last_error() or ""), ops
    n += 1
for images, count, fmt in ((arr, 0, 83), (None, 1, 83), (arr, 1, 0), (arr, 1, 98)):       # itwCompressImageChainEx's refusals, with valid ops
    L.itwClearError()
    assert L.itwCompressNormalMapChain(images, count, out.ctypes.data, fmt, None, 7, None, None) is False and itw_amd.last_error()
    n += 1
assert not out.any()
print("rejected", n)
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "rejected 8"


def _want_faces(img):
    h, w = img.shape[:2]
    vertical = w < h
    fw, fh = (w // 3, h // 4) if vertical else (w // 4, h // 3)
    cells = [(2, 1), (0, 1), (1, 0), (1, 2), (1, 1), (1, 3) if vertical else (3, 1)]
    return [img[r * fh:(r + 1) * fh, c * fw:(c + 1) * fw] for c, r in cells]


@pytest.mark.parametrize("h,w", [(24, 32), (32, 24), (15, 20), (20, 15), (26, 35), (35, 26), (3, 4), (4, 3), (3, 3)])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_cube_cross_faces_are_numpy_slices(itw, h, w, dtype):
    """Horizontal and vertical crosses with faces of 8 and 5, sizes that do not divide (26 x 35: the quotients truncate), the smallest
    crosses, and a square (3 x 3: not vertical, so a horizontal cross of 0-wide faces is refused)."""
    rng = np.random.default_rng(h * 100 + w)
    canvas = rng.integers(0, 256, (h, w + 2, 4)).astype(dtype)      # two texels of row padding: the views keep the cross's stride
    img = canvas[:, :w]
    if (h, w) == (3, 3):
        with pytest.raises(ValueError):
            itw.cube_cross_faces(img)
        return
    faces = itw.cube_cross_faces(img)
    want = _want_faces(img)
    assert len(faces) == 6
    for f, v in zip(faces, want):
        assert f.shape == v.shape and f.shape[0] >= 1 and f.shape[1] >= 1
        assert f.ctypes.data == v.ctypes.data and f.strides == v.strides and np.array_equal(f, v)


def test_cube_cross_refuses_null_and_small(itw):
    L = itw.lib()
    S = itw.RgbaSurface
    img = np.zeros((12, 16, 4), np.uint8)
    faces = (S * 6)()
    ok = S(img.ctypes.data, 16, 12, 64)
    assert L.itwCubeCrossFaces(C.byref(ok), 4, faces) == 0
    assert (faces[0].width, faces[0].height, faces[0].stride, faces[0].ptr) == (4, 4, 64, img.ctypes.data + 4 * 64 + 8 * 4)
    assert L.itwCubeCrossFaces(None, 4, faces) == -1
    assert L.itwCubeCrossFaces(C.byref(ok), 4, None) == -1
    assert L.itwCubeCrossFaces(C.byref(S(None, 16, 12, 64)), 4, faces) == -1
    assert L.itwCubeCrossFaces(C.byref(ok), 3, faces) == -1
    for w, h in ((3, 3), (4, 2), (2, 4), (3, 2), (0, 0), (2, 3)):
        assert L.itwCubeCrossFaces(C.byref(S(img.ctypes.data, w, h, 64)), 4, faces) == -1, (w, h)
