"""itwPrepareNormalMapChain on the device (include/itw_dispatch.h; csrc/normal_prep.hip, normal_prep.hpp) against the numpy checker of
tests/_normal_prep.py, bit for bit: every RGB triple of the 8-bit normalise (and the SHA-256 of the reference's own loop over them,
tests/golden/normal_prep_sha256.json), every code under the flips, every finite half under the 16-bit stages, the geometry (odd sizes, views
into a canvas whose rows are only 4-byte aligned, guard bytes) and the host-pointer route."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import _normal_prep as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _dev(gpu, a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(gpu)


def _host(t, like):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(like.dtype)


def _run(itw, gpu, img, ops):
    """img (H, W, 4) uint8 / uint16 -> the device's in-place result as numpy"""
    t = _dev(gpu, np.ascontiguousarray(img))
    itw.prepare_normal_map(t, ops=ops)
    return _host(t, img)


@pytest.fixture(scope="module")
def triples():
    img = N.all_triples()
    return img, N.prepare_rgba8(img, N.NORMALIZE)


def test_exhaustive_8bit_normalise(itw, gpu, triples):
    img, want = triples
    got = _run(itw, gpu, img, N.NORMALIZE)
    bad = np.nonzero((got != want).any(axis=2).reshape(-1))[0]
    assert bad.size == 0, (bad.size, [(int(i), img.reshape(-1, 4)[i].tolist(), got.reshape(-1, 4)[i].tolist(), want.reshape(-1, 4)[i].tolist()) for i in bad[:4]])
    assert np.array_equal(got[..., 3], img[..., 3])
    with open(os.path.join(ROOT, "tests", "golden", "normal_prep_sha256.json")) as f:
        pin = json.load(f)["normalize_rgb8_all_triples"]
    assert hashlib.sha256(np.ascontiguousarray(got[..., :3]).tobytes()).hexdigest() == pin


@pytest.mark.parametrize("ops", [0, 1, 2, 3])
def test_8bit_flips_over_every_code(itw, gpu, ops):
    rng = np.random.default_rng(ops)
    img = rng.integers(0, 256, (16, 16, 4), dtype=np.uint8)
    img[..., 0] = np.arange(256, dtype=np.uint8).reshape(16, 16)
    img[..., 1] = np.arange(256, dtype=np.uint8).reshape(16, 16)[::-1]
    got = _run(itw, gpu, img, ops)
    assert np.array_equal(got, N.prepare_rgba8(img, ops))
    assert np.array_equal(got[..., 2:], img[..., 2:])
    assert np.array_equal(got[..., 0], 255 - img[..., 0] if ops & 1 else img[..., 0])
    assert np.array_equal(got[..., 1], 255 - img[..., 1] if ops & 2 else img[..., 1])


@pytest.mark.parametrize("ops", [5, 6, 7])
def test_all_ops_together_8bit(itw, gpu, ops):
    img = np.random.default_rng(70 + ops).integers(0, 256, (256, 256, 4), dtype=np.uint8)
    got = _run(itw, gpu, img, ops)
    assert np.array_equal(got, N.prepare_rgba8(img, ops))
    assert np.array_equal(got[..., 3], img[..., 3])


def _finite_halves():
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    return h[(h & 0x7C00) != 0x7C00]                      # 63 488 patterns: no infinity, no NaN


# (G, B) pairs: zeros, +-0, the smallest denormal, 1.0, 65504, mixed signs
PAIRS = [(0x0000, 0x0000), (0x8000, 0x0000), (0x0000, 0x8000), (0x0001, 0x8001), (0x3C00, 0x3C00), (0x7BFF, 0x7BFF), (0xBC00, 0x3800), (0x4500, 0xFBFF)]


def _half_sweep(swap):
    r = _finite_halves()
    img = np.empty((len(PAIRS), r.size, 4), np.uint16)
    for k, (g, b) in enumerate(PAIRS):
        img[k, :, 0] = r
        img[k, :, 1] = g
        img[k, :, 2] = b
    img[..., 3] = (np.arange(r.size) * 40503).astype(np.uint16)[None, :]
    if swap:
        img[..., [0, 1]] = img[..., [1, 0]]
    return img


def _assert_half(got, want, img):
    bad = np.nonzero((got != want).any(axis=-1).reshape(-1))[0]
    assert bad.size == 0, (bad.size, [([hex(v) for v in img.reshape(-1, 4)[i]], [hex(v) for v in got.reshape(-1, 4)[i]], [hex(v) for v in want.reshape(-1, 4)[i]]) for i in bad[:4]])


@pytest.mark.parametrize("swap", [False, True])
def test_rgba16f_normalise_over_every_finite_half(itw, gpu, swap):
    img = _half_sweep(swap)
    want = N.prepare_rgba16f(img, N.NORMALIZE)
    assert not (((want[..., :3] & 0x7C00) == 0x7C00) & ((want[..., :3] & 0x03FF) != 0)).any()       # finite inputs: no NaN comes out, every case is compared
    got = _run(itw, gpu, img, N.NORMALIZE)
    _assert_half(got, want, img)
    assert np.array_equal(got[..., 3], img[..., 3])


def test_rgba16f_random_finite_triples_all_ops(itw, gpu):
    rng = np.random.default_rng(16)
    fin = _finite_halves()
    img = fin[rng.integers(0, fin.size, (1024, 1024, 4))]
    for ops in (4, 7):
        want = N.prepare_rgba16f(img, ops)
        nan = ((want[..., :3] & 0x7C00) == 0x7C00) & ((want[..., :3] & 0x03FF) != 0)
        ok = ~nan.any(axis=-1)                                  # (a flipped 65504 stays finite too: nothing is left out in practice)
        got = _run(itw, gpu, img, ops)
        _assert_half(got[ok], want[ok], img[ok])
        assert ok.mean() > 0.999
        assert np.array_equal(got[..., 3], img[..., 3])


@pytest.mark.parametrize("ops", [1, 2, 3])
def test_rgba16f_flips_over_every_finite_half(itw, gpu, ops):
    r = _finite_halves()
    img = np.zeros((1, r.size, 4), np.uint16)
    img[0, :, 0] = r
    img[0, :, 1] = r[::-1]
    img[0, :, 2] = r
    img[0, :, 3] = r[::-1]
    got = _run(itw, gpu, img, ops)
    _assert_half(got, N.prepare_rgba16f(img, ops), img)
    assert np.array_equal(got[..., 2:], img[..., 2:])


def test_zero_vector_gives_the_default_normal(itw, gpu):
    img = np.full((3, 5, 4), 128, np.uint8)
    img[..., 3] = 9
    got = _run(itw, gpu, img, N.NORMALIZE)
    assert (got == np.array([128, 128, 255, 9], np.uint8)).all()
    h = np.zeros((2, 4, 4), np.uint16)
    for i in range(8):
        h.reshape(-1, 4)[i, :3] = [0x8000 if i & 1 else 0, 0x8000 if i & 2 else 0, 0x8000 if i & 4 else 0]
    h[..., 3] = 0x1234
    got = _run(itw, gpu, h, N.NORMALIZE)
    assert (got == np.array([0, 0, 0x3C00, 0x1234], np.uint16)).all()


SIZES = [(1, 1), (3, 2), (7, 5), (64, 64), (66, 130)]      # (height, width)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("on_device", [True, False])
def test_geometry_views_and_guard_bytes(itw, gpu, dtype, on_device):
    """One call over five images; three are views into a canvas whose rows are texel aligned but not 16-byte aligned; everything around the
    images and in their rows' padding stays as it was."""
    import torch
    rng = np.random.default_rng(5)
    es = np.dtype(dtype).itemsize
    canvas_w = 203 if es == 1 else 201                       # row bytes 812 / 1608: multiples of 4 / 8, not of 16
    canvas = rng.integers(0, 256 if es == 1 else 0x7C00, (150, canvas_w, 4)).astype(dtype)
    lone = [rng.integers(0, 256 if es == 1 else 0x7C00, (h, w + 3, 4)).astype(dtype) for h, w in SIZES[:2]]       # own buffers, 3 texels of row padding
    before_c, before_l = canvas.copy(), [a.copy() for a in lone]
    spots = [(1, 1), (70, 3), (75, 69)]
    if on_device:
        tc = _dev(gpu, canvas)
        tl = [_dev(gpu, a) for a in lone]
    else:
        tc, tl = canvas, lone
    views = [tl[i][:h, :w] for i, (h, w) in enumerate(SIZES[:2])]
    views += [tc[y:y + h, x:x + w] for (y, x), (h, w) in zip(spots, SIZES[2:])]
    itw.prepare_normal_map(views, ops=7)
    if on_device:
        torch.cuda.synchronize()
        canvas = tc.cpu().numpy().view(dtype)
        lone = [t.cpu().numpy().view(dtype) for t in tl]
    want_c, want_l = before_c.copy(), [a.copy() for a in before_l]
    for i, (h, w) in enumerate(SIZES[:2]):
        want_l[i][:h, :w] = N.prepare(before_l[i][:h, :w], 7)
    for (y, x), (h, w) in zip(spots, SIZES[2:]):
        want_c[y:y + h, x:x + w] = N.prepare(before_c[y:y + h, x:x + w], 7)
    assert np.array_equal(canvas, want_c)
    for a, b in zip(lone, want_l):
        assert np.array_equal(a, b)


def test_host_pointers_give_the_device_result(itw, gpu):
    img = np.random.default_rng(8).integers(0, 256, (37, 53, 4), dtype=np.uint8)
    dev = _run(itw, gpu, img, 7)
    host = img.copy()
    itw.prepare_normal_map(host, ops=7)
    assert np.array_equal(host, dev) and np.array_equal(host, N.prepare_rgba8(img, 7))


def test_no_ops_and_no_images_write_nothing(itw, gpu):
    img = np.random.default_rng(9).integers(0, 256, (8, 8, 4), dtype=np.uint8)
    t = _dev(gpu, img)
    itw.prepare_normal_map(t, ops=0)
    assert np.array_equal(_host(t, img), img)
    s = itw.RgbaSurface(t.data_ptr(), 8, 8, 32)
    assert itw.lib().itwPrepareNormalMapChain(C.byref(s), 0, 4, 7) == 0
    assert np.array_equal(_host(t, img), img)


def test_mixed_host_and_device_pointers_are_refused(itw, gpu):
    img = np.zeros((4, 4, 4), np.uint8)
    t = _dev(gpu, img)
    arr = (itw.RgbaSurface * 2)(itw.RgbaSurface(t.data_ptr(), 4, 4, 16), itw.RgbaSurface(img.ctypes.data, 4, 4, 16))
    assert itw.lib().itwPrepareNormalMapChain(C.cast(arr, C.c_void_p), 2, 4, 4) == -1
    assert not img.any() and not _host(t, img).any()
