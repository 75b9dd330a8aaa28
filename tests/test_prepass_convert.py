"""Photoshop-buffer -> encoder-surface conversions (IntelPlugin.cpp:741-810, :291-366): the oracle's restatement against
independent numpy formulas (CPU), and the device kernels of csrc/convert.hip against the oracle (GPU).  Exact for every
path -- since round 6 also 32-bit -> 8-bit with gamma: the kernel counts the code thresholds of the reference's own function
(csrc/gamma_thresholds.h) instead of calling a device pow().

float -> half is pinned to IEEE 754 round to nearest even (oracle/prepass.c): the restatement is swept against
numpy over every float of the two ranges where a software rule can differ and over every rounding decision point (tests/_half_points.py),
the kernel over the decision points, a strided pass of the ranges and the special values; the 8- and 16-bit sources are exhaustive."""
import ctypes as C
import os

import numpy as np
import pytest

import _half_points as HP
from _guarded import guarded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle8(oracle, src, depth, planes, has_alpha, gamma, w, h):
    out = np.zeros((h, w, 4), dtype=np.uint8)
    oracle.lib().oracle_convert_rgba8(src.ctypes.data_as(C.c_void_p), depth, planes, has_alpha, gamma, w, h, out.ctypes.data_as(C.c_void_p))
    return out


def _oracle16(oracle, src, depth, planes, has_alpha, w, h):
    out = np.zeros((h, w, 4), dtype=np.uint16)
    oracle.lib().oracle_convert_rgba16f(src.ctypes.data_as(C.c_void_p), depth, planes, has_alpha, w, h, out.ctypes.data_as(C.c_void_p))
    return out


def _source(rng, depth, planes, w, h):
    if depth == 8:
        return rng.integers(0, 256, size=(h, w, planes), dtype=np.uint8)
    if depth == 16:
        s = rng.integers(0, 32769, size=(h, w, planes)).astype(np.uint16)       # Photoshop's 0..32768
        s.reshape(-1)[:6] = [0, 1, 32767, 32768, 40000, 65535]
        return s
    s = rng.random((h, w, planes), dtype=np.float32) * np.float32(1.3) - np.float32(0.1)   # some < 0 and > 1
    s.reshape(-1)[:6] = [0.0, 1.0, 0.5, 1e-8, 0.999999, 65504.0]
    return s


def test_oracle_conversions_match_the_formulas(oracle):
    rng = np.random.default_rng(4)
    w, h = 37, 11
    for planes, alpha in ((1, 0), (3, 0), (4, 1), (4, 0)):
        s8 = _source(rng, 8, planes, w, h)
        got = _oracle8(oracle, s8, 8, planes, alpha, 0, w, h)
        want = np.zeros((h, w, 4), np.uint8); want[..., 3] = 255
        want[..., :min(planes, 3)] = s8[..., :min(planes, 3)]
        if alpha: want[..., 3] = s8[..., 3]
        assert np.array_equal(got, want)
        s16 = _source(rng, 16, planes, w, h)
        got = _oracle8(oracle, s16, 16, planes, alpha, 0, w, h)
        conv = np.where(s16 > 32768, 255, (s16.astype(np.int64) * 255) >> 15).astype(np.uint8)
        want = np.zeros((h, w, 4), np.uint8); want[..., 3] = 255
        want[..., :min(planes, 3)] = conv[..., :min(planes, 3)]
        if alpha: want[..., 3] = conv[..., 3]
        assert np.array_equal(got, want)
        got16 = _oracle16(oracle, s8, 8, planes, alpha, w, h)
        conv = (s8.astype(np.float32) / np.float32(255)).astype(np.float16).view(np.uint16)
        want = np.zeros((h, w, 4), np.uint16); want[..., 3] = 0x3C00
        want[..., :min(planes, 3)] = conv[..., :min(planes, 3)]
        if alpha: want[..., 3] = conv[..., 3]
        assert np.array_equal(got16, want)
        s32 = _source(rng, 32, planes, w, h)
        got16 = _oracle16(oracle, s32, 32, planes, alpha, w, h)
        conv = s32.astype(np.float16).view(np.uint16)                 # IEEE round to nearest even = XMConvertFloatToHalf in range
        want = np.zeros((h, w, 4), np.uint16); want[..., 3] = 0x3C00
        want[..., :min(planes, 3)] = conv[..., :min(planes, 3)]
        if alpha: want[..., 3] = conv[..., 2]                         # the reference reads plane 2 (IntelPlugin.cpp:361)
        assert np.array_equal(got16, want)


def _half_via_oracle(oracle, bits):
    """Float bit patterns through oracle_convert_rgba16f as a one-plane source: the half bit patterns of the red channel."""
    src = np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)
    out = _oracle16(oracle, src, 32, 1, 0, src.size, 1).reshape(-1, 4)
    assert not out[:, 1:3].any() and (out[:, 3] == 0x3C00).all()
    return out[:, 0]


def _assert_same_halves(got, want, bits, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, [(hex(int(bits[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]])


def test_oracle_float_to_half_is_ieee_round_to_nearest_even_wherever_a_rule_can_differ(oracle):
    """f32_to_f16 of oracle/prepass.c against numpy's astype(float16), all ==, in both signs: every float of 2^-25 .. 2^-14 (half
    denormals; 92 274 720 floats per sign) and of 65280 .. 65536 (65 552), and every half and every midpoint between two halves +-3
    floats (444 413).  The rule the file restated before -- sticky bits of a denormal dropped, inf above 65504 -- differs from IEEE at
    6 144 + 4 095 floats per sign of the two ranges, at 1 024 + 6 of the structured points, and nowhere else among finite inputs."""
    assert _half_via_oracle(oracle, np.array([0x33000001, 0x477fe001, 0xb3000001, 0xc77fe001], np.uint32)).tolist() == [0x0001, 0x7BFF, 0x8001, 0xFBFF]
    s = HP.structured()
    differs = HP.legacy_half_bits(s) != HP.ieee_half_bits(s)                       # the point set tells the two rules apart ...
    assert (int((differs & (s < 0x38800000)).sum()), int((differs & (s >= 0x38800000)).sum())) == HP.LEGACY_DIFFERS_STRUCTURED
    s = HP.both_signs(s)
    _assert_same_halves(_half_via_oracle(oracle, s), HP.ieee_half_bits(s), s, "structured")             # ... and the oracle is the IEEE one
    # numpy raises the underflow / overflow flag per element in these ranges (0.1 us each): the chunks go through a few threads, both the
    # cast and the oracle call release the interpreter lock
    from concurrent.futures import ThreadPoolExecutor
    chunk = 1 << 21
    jobs = [(sign, a, min(a + chunk, hi)) for sign in (0, 0x80000000) for lo, hi in (HP.DENORMAL_RANGE, HP.TOP_RANGE) for a in range(lo, hi, chunk)]

    def one(job):
        sign, a, b = job
        bits = (np.arange(a, b, dtype=np.int64) | sign).astype(np.uint32)
        _assert_same_halves(_half_via_oracle(oracle, bits), HP.ieee_half_bits(bits), bits, (hex(sign), hex(a)))
        return b - a

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        assert sum(pool.map(one, jobs)) == 2 * (92_274_720 + 65_552)


def test_legacy_rule_differs_from_ieee_only_inside_the_swept_ranges():
    """Why those two ranges: between them (half normals, where both rules are the same code) and outside them (flushes to 0, inf) the
    legacy restatement equals IEEE on every 997th float and next to every boundary, so the exhaustive sweep above leaves nothing out."""
    edges = np.array([0, 0x00800000, HP.DENORMAL_RANGE[0], HP.DENORMAL_RANGE[1], HP.TOP_RANGE[0], HP.TOP_RANGE[1], 0x7f7fffff, 0x7f800000], np.int64)
    near = (edges[:, None] + np.arange(-16, 17)[None, :]).reshape(-1)
    outside = np.concatenate([np.arange(0, HP.DENORMAL_RANGE[0], 997), np.arange(HP.DENORMAL_RANGE[1], HP.TOP_RANGE[0], 997),
                              np.arange(HP.TOP_RANGE[1], 0x7f800001, 997), near])
    outside = outside[(outside >= 0) & (outside <= 0x7f800000)]
    outside = outside[((outside < HP.DENORMAL_RANGE[0]) | (outside >= HP.DENORMAL_RANGE[1])) & ((outside < HP.TOP_RANGE[0]) | (outside >= HP.TOP_RANGE[1]))]
    bits = HP.both_signs(outside.astype(np.uint32))
    assert np.array_equal(HP.legacy_half_bits(bits), HP.ieee_half_bits(bits))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 16, 32])
def test_device_conversions_match_the_oracle(itw, gpu, oracle, depth):
    import torch
    rng = np.random.default_rng(depth)
    w, h = 203, 57
    L = itw.lib()
    L.itwSetStream(torch.cuda.current_stream().cuda_stream)
    for planes, alpha in ((1, 0), (2, 0), (3, 0), (4, 1), (4, 0)):
        src = _source(rng, depth, planes, w, h)
        d_src = torch.from_numpy(src.view(np.int16) if depth == 16 else src).to(gpu)
        for gamma in ((0, 1) if depth == 32 else (0,)):
            d8 = torch.zeros((h, w, 4), dtype=torch.uint8, device=gpu)
            assert L.itwConvertToRGBA8Device(d_src.data_ptr(), depth, planes, alpha, gamma, w, h, d8.data_ptr()) == 0
            torch.cuda.synchronize()
            got, want = d8.cpu().numpy(), _oracle8(oracle, src, depth, planes, alpha, gamma, w, h)
            assert np.array_equal(got, want), (depth, planes, alpha, gamma)       # the gamma route too: thresholds, not a device pow
        d16 = torch.zeros((h, w, 4), dtype=torch.int16, device=gpu)
        assert L.itwConvertToRGBA16FDevice(d_src.data_ptr(), depth, planes, alpha, w, h, d16.data_ptr()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(d16.cpu().numpy().view(np.uint16), _oracle16(oracle, src, depth, planes, alpha, w, h))
    assert L.itwConvertToRGBA8Device(d_src.data_ptr(), 12, 3, 0, 0, w, h, d8.data_ptr()) == -1
    assert L.itwConvertToRGBA8Device(d_src.data_ptr(), depth, 3, 1, 0, w, h, d8.data_ptr()) == -1   # alpha needs plane 3


def _thresholds():
    import re
    text = open(os.path.join(ROOT, "intel-texture-works-plugin_amd", "csrc", "gamma_thresholds.h")).read()
    return np.array([int(x, 16) for x in re.findall(r"0x([0-9a-f]{8})u", text)], dtype=np.uint32)


def test_gamma_thresholds_are_the_code_boundaries_of_the_oracle(oracle):
    """csrc/gamma_thresholds.h (generated from the reference's ConvertTo8Bit compiled here): entry c is the smallest float whose code is >= c --
    checked against oracle/prepass.c (the same C library pow) at every threshold and its neighbours, increasing, and [255] <= 1.0."""
    thr = _thresholds()
    assert thr.size == 256 and thr[0] == 0 and np.all(np.diff(thr[1:].astype(np.int64)) > 0) and thr[255] <= np.float32(1.0).view(np.uint32)
    bits = (thr[1:, None].astype(np.int64) + np.arange(-2, 3)[None, :]).astype(np.uint32)          # 255 x 5 floats around the crossings
    src = bits.view(np.float32).reshape(-1)
    got = _oracle8(oracle, np.ascontiguousarray(src), 32, 1, 0, 1, src.size, 1)[..., 0].reshape(255, 5)
    c = np.arange(1, 256)[:, None]
    assert np.array_equal(got >= c, np.broadcast_to(np.arange(-2, 3)[None, :] >= 0, (255, 5)))


@pytest.mark.gpu
def test_gamma_route_is_bit_exact_at_every_code_boundary_and_for_special_values(itw, gpu, oracle):
    """The 32-bit -> 8-bit gamma route (IntelPlugin.h:66-73) on the device equals the C library route bit for bit: every threshold +-3 floats,
    two million random floats of [0, 1.2), zeros of both signs, denormals, negatives, values above 1, infinities and NaN."""
    import torch
    thr = _thresholds()
    rng = np.random.default_rng(32)
    edge = (thr[1:, None].astype(np.int64) + np.arange(-3, 4)[None, :]).astype(np.uint32).view(np.float32).reshape(-1)
    special = np.array([0.0, -0.0, 1e-45, 1e-40, -1e-40, -1.0, -np.inf, 1.0, 1.0000001, 2.0, 1e30, np.inf, np.nan, 0.5, 0.2176, 0.9999999], dtype=np.float32)
    src = np.concatenate([edge, special, rng.random(2_000_000, dtype=np.float32) * np.float32(1.2),
                          np.exp(rng.uniform(-40, 0.1, 200_000)).astype(np.float32)])
    src = np.ascontiguousarray(src[:src.size // 4 * 4])
    n = src.size
    d_src = torch.from_numpy(src).to(gpu)
    d8 = torch.zeros((1, n, 4), dtype=torch.uint8, device=gpu)
    itw.lib().itwSetStream(torch.cuda.current_stream().cuda_stream)
    assert itw.lib().itwConvertToRGBA8Device(d_src.data_ptr(), 32, 1, 0, 1, n, 1, d8.data_ptr()) == 0
    torch.cuda.synchronize()
    got = d8.cpu().numpy()[0, :, 0]
    want = _oracle8(oracle, src, 32, 1, 0, 1, n, 1)[0, :, 0]
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:5], src[bad[:5]], got[bad[:5]], want[bad[:5]])


# ---- the device kernels, swept ---------------------------------------------------------------------------------------------------------

LAYOUTS = ((1, 0), (2, 0), (3, 0), (4, 0), (4, 1))


def _upload(gpu, src):
    import torch
    return torch.from_numpy(src.view(np.int16) if src.dtype == np.uint16 else src).to(gpu)


def _device8(itw, gpu, src, depth, planes, alpha, gamma, w, h, d_src=None):
    import torch
    d_src = _upload(gpu, src) if d_src is None else d_src
    d8 = torch.full((h, w, 4), 0x5A, dtype=torch.uint8, device=gpu)
    itw.lib().itwSetStream(torch.cuda.current_stream().cuda_stream)
    assert itw.lib().itwConvertToRGBA8Device(d_src.data_ptr(), depth, planes, alpha, gamma, w, h, d8.data_ptr()) == 0
    torch.cuda.synchronize()
    return d8.cpu().numpy()


def _device16(itw, gpu, src, depth, planes, alpha, w, h, d_src=None):
    import torch
    d_src = _upload(gpu, src) if d_src is None else d_src
    d16 = torch.full((h, w, 4), 0x5A5A, dtype=torch.int16, device=gpu)
    itw.lib().itwSetStream(torch.cuda.current_stream().cuda_stream)
    assert itw.lib().itwConvertToRGBA16FDevice(d_src.data_ptr(), depth, planes, alpha, w, h, d16.data_ptr()) == 0
    torch.cuda.synchronize()
    return d16.cpu().numpy().view(np.uint16)


def _formula(src, depth, planes, alpha, half):
    """The conversions as numpy formulas, independent of oracle/prepass.c (8- and 16-bit sources; float -> half is numpy's IEEE cast)."""
    if half:
        f = src.astype(np.float32) / np.float32(255) if depth == 8 else (src.astype(np.float64) / 32768.0).astype(np.float32)
        conv = f.astype(np.float16).view(np.uint16)
    else:
        conv = src if depth == 8 else np.where(src > 32768, 255, (src.astype(np.int64) * 255) >> 15).astype(np.uint8)
    want = np.zeros(src.shape[:2] + (4,), conv.dtype)
    want[..., 3] = 0x3C00 if half else 255
    want[..., :min(planes, 3)] = conv[..., :min(planes, 3)]
    if alpha:
        want[..., 3] = conv[..., 3]
    return want


HALF_SPECIALS = [0x00000000, 0x80000000,                                           # +-0
                 0x32ffffff, 0x33000000, 0x33000001, 0xb2ffffff, 0xb3000000, 0xb3000001,       # +-2^-25 (the tie between 0 and the smallest half)
                 0x337fffff, 0x33800000, 0x33800001, 0xb3800000,                   # +-2^-24, the smallest half
                 0x00800000, 0x80800000,                                           # +-FLT_MIN
                 0x00000001, 0x00400000, 0x007fffff, 0x80000001, 0x807fffff,       # float denormals
                 0x387fffff, 0x38800000, 0xb87fffff,                               # the smallest half normal, 2^-14
                 0x477fe000, 0x477fe001, 0x477fefff, 0x477ff000, 0x477ff001,       # 65504, ..., the last float below 65520, 65520
                 0xc77fe000, 0xc77fefff, 0xc77ff000,
                 0x47800000, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000]       # 65536, +-FLT_MAX, +-inf
HALF_NANS = [0x7fc00000, 0x7f800001, 0x7f801000, 0x7fa00000, 0x7fffffff,           # quiet, signalling, payload below the half's mantissa, ...
             0xffc00000, 0xff800001, 0xff801000, 0xffa00000, 0xffffffff]


@pytest.mark.gpu
def test_device_float_to_half_is_ieee_at_every_rounding_decision(itw, gpu, oracle):
    """32-bit -> half on the device, one plane, one launch of 3.8 M pixels: every half and every midpoint between two halves +-3 floats in
    both signs (888 826), every 67th float of the half-denormal range and every float of 65280 .. 65536 in both signs, and the special
    values -- equal to oracle/prepass.c AND to numpy's astype(float16).  Excluded from ==: exactly the 10 NaN inputs (five payloads, both
    signs), which must come out as NaN; which NaN is unpinned."""
    start = np.random.default_rng(67).integers(0, 67)
    bits = np.concatenate([HP.both_signs(HP.structured()), HP.both_signs(HP.whole_range(HP.DENORMAL_RANGE, 67, int(start))),
                           HP.both_signs(HP.whole_range(HP.TOP_RANGE)), np.array(HALF_SPECIALS, np.uint32), np.array(HALF_NANS, np.uint32)])
    n = bits.size
    assert 3_500_000 < n < 4_100_000
    src = bits.view(np.float32)
    got = _device16(itw, gpu, src, 32, 1, 0, n, 1).reshape(n, 4)
    assert not got[:, 1:3].any() and (got[:, 3] == 0x3C00).all()
    got = got[:, 0]
    nan = np.isnan(src)
    assert int(nan.sum()) == len(HALF_NANS) == 10 and nan[-10:].all()
    assert ((got[nan] & 0x7c00) == 0x7c00).all() and ((got[nan] & 0x03ff) != 0).all(), [hex(v) for v in got[nan]]
    keep = ~nan
    want = _half_via_oracle(oracle, bits)
    ieee = HP.ieee_half_bits(bits)
    print(f"float -> half on the device: {int((got[keep] != want[keep]).sum())} of {int(keep.sum())} points differ from the oracle, "
          f"{int((got[keep] != ieee[keep]).sum())} from numpy")
    _assert_same_halves(got[keep], want[keep], bits[keep], "device vs oracle")
    _assert_same_halves(got[keep], ieee[keep], bits[keep], "device vs numpy")


def _rolled_ramp(depth, planes):
    """Every value of an 8- / 16-bit source in every plane: the ramp 0 .. 255 / 65535, rolled by another offset in each plane."""
    n = 1 << depth
    ramp = np.arange(n, dtype=np.uint8 if depth == 8 else np.uint16)
    src = np.stack([np.roll(ramp, p * (n // 3 + 1)) for p in range(planes)], axis=1).reshape(1, n, planes)
    assert all(np.array_equal(np.sort(src[0, :, p]), ramp) for p in range(planes))
    return np.ascontiguousarray(src)


@pytest.mark.gpu
@pytest.mark.parametrize("planes,alpha", LAYOUTS, ids=[f"{p}-planes-alpha{a}" for p, a in LAYOUTS])
@pytest.mark.parametrize("depth", [8, 16])
def test_device_conversions_of_every_8_and_16_bit_value_in_every_plane(itw, gpu, oracle, depth, planes, alpha):
    """All 256 / 65 536 source values (the 32 767 above Photoshop's 32768 too) in every plane of every layout, to both targets: equal to the
    oracle and to the numpy formulas."""
    src = _rolled_ramp(depth, planes)
    n = src.shape[1]
    d_src = _upload(gpu, src)
    got8 = _device8(itw, gpu, src, depth, planes, alpha, 0, n, 1, d_src)
    assert np.array_equal(got8, _oracle8(oracle, src, depth, planes, alpha, 0, n, 1))
    assert np.array_equal(got8, _formula(src, depth, planes, alpha, False))
    got16 = _device16(itw, gpu, src, depth, planes, alpha, n, 1, d_src)
    assert np.array_equal(got16, _oracle16(oracle, src, depth, planes, alpha, n, 1))
    assert np.array_equal(got16, _formula(src, depth, planes, alpha, True))


GAMMA_TEST_SPECIALS = [0.0, -0.0, 1e-45, 1e-40, -1e-40, -1.0, -np.inf, 1.0, 1.0000001, 2.0, 1e30, np.inf, np.nan, 0.5, 0.2176, 0.9999999]


@pytest.mark.gpu
def test_device_float_to_byte_without_gamma_at_every_code_boundary(itw, gpu, oracle):
    """32-bit -> 8-bit without gamma is (unsigned char)(double(v) * 255) behind the clamps (IntelPlugin.h:41-48): the code changes next to k / 255,
    so the floats at k / 255 +-3 for k = 0 .. 255 (below 0: the negative floats next to -0), and the special values of the gamma test."""
    centre = (np.arange(256, dtype=np.float64) / 255).astype(np.float32).view(np.uint32).astype(np.int64)
    edge = (centre[:, None] + np.arange(-3, 4)[None, :]).reshape(-1)
    edge = np.where(edge < 0, 0x80000000 - edge, edge).astype(np.uint32)            # -1, -2, -3 floats from +0: -0 is 0, so 0x80000001 ..
    src = np.ascontiguousarray(np.concatenate([edge.view(np.float32), np.array(GAMMA_TEST_SPECIALS, np.float32)]))
    n = src.size
    assert n == 256 * 7 + 16
    got = _device8(itw, gpu, src, 32, 1, 0, 0, n, 1)
    want = _oracle8(oracle, src, 32, 1, 0, 0, n, 1)
    bad = np.flatnonzero((got != want).any(axis=-1).reshape(-1))
    assert bad.size == 0, (bad[:5], src[bad[:5]], got.reshape(n, 4)[bad[:5]], want.reshape(n, 4)[bad[:5]])
    assert len(set(want[0, :256 * 7, 0].tolist())) == 256                           # the points do straddle every code


@pytest.mark.gpu
def test_device_float_to_half_takes_alpha_from_plane_2_of_a_three_plane_source(itw, gpu, oracle):
    """planes 3 with has_alpha is a legal 32-bit -> half call: ConvertToBC6From32Bit reads its alpha at index + 2 (IntelPlugin.cpp:361)."""
    rng = np.random.default_rng(361)
    w, h = 131, 5
    src = (rng.random((h, w, 3), dtype=np.float32) * np.float32(4) - np.float32(1))
    got = _device16(itw, gpu, src, 32, 3, 1, w, h)
    assert np.array_equal(got, _oracle16(oracle, src, 32, 3, 1, w, h))
    want = src.astype(np.float16).view(np.uint16)
    assert np.array_equal(got[..., :3], want) and np.array_equal(got[..., 3], want[..., 2])


@pytest.mark.gpu
@pytest.mark.parametrize("planes", [1, 3])
def test_device_conversions_from_an_8_bit_source_at_an_odd_address(itw, gpu, oracle, planes):
    """A byte source has no alignment: a plane pointer one byte past an aligned address, to both targets."""
    import torch
    w, h = 173, 3
    src = np.random.default_rng(planes).integers(0, 256, size=(h, w, planes), dtype=np.uint8)
    base = torch.zeros(src.size + 1, dtype=torch.uint8, device=gpu)
    d_src = base[1:]
    d_src.copy_(torch.from_numpy(src.reshape(-1)))
    assert d_src.data_ptr() % 2 == 1
    assert np.array_equal(_device8(itw, gpu, src, 8, planes, 0, 0, w, h, d_src), _oracle8(oracle, src, 8, planes, 0, 0, w, h))
    assert np.array_equal(_device16(itw, gpu, src, 8, planes, 0, w, h, d_src), _oracle16(oracle, src, 8, planes, 0, w, h))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 16, 32])
@pytest.mark.parametrize("w,h", [(1, 1), (255, 1), (256, 1), (257, 1), (37, 11)], ids=["1", "255", "256", "257", "37x11"])
def test_device_conversions_write_exactly_their_pixels_around_the_block_size(itw, gpu, oracle, w, h, depth):
    """One lane per pixel in blocks of 256: one pixel, one short of a block, a block, one lane into a second block, and 407 = 37 x 11 pixels.
    The destination lies between guard bands (tests/_guarded.py); four planes with alpha, and for 32-bit -> half also three."""
    import torch
    L = itw.lib()
    L.itwSetStream(torch.cuda.current_stream().cuda_stream)
    src = np.ascontiguousarray(_source(np.random.default_rng(w * h + depth), depth, 4, max(w, 6), h)[:, :w])
    d_src = _upload(gpu, src)
    out8, out16 = guarded(w * h * 4, device=gpu), guarded(w * h * 8, device=gpu)
    for gamma in ((0, 1) if depth == 32 else (0,)):
        out8.refill()
        assert L.itwConvertToRGBA8Device(d_src.data_ptr(), depth, 4, 1, gamma, w, h, out8.ptr) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out8.host().reshape(h, w, 4), _oracle8(oracle, src, depth, 4, 1, gamma, w, h)), gamma
        out8.check(f"convert8 {w}x{h} depth {depth} gamma {gamma}")
    layouts = [(4, 1, src, d_src)]
    if depth == 32:
        src3 = np.ascontiguousarray(src[..., :3])
        layouts.append((3, 1, src3, _upload(gpu, src3)))
    for planes, alpha, s, d in layouts:
        out16.refill()
        assert L.itwConvertToRGBA16FDevice(d.data_ptr(), depth, planes, alpha, w, h, out16.ptr) == 0
        torch.cuda.synchronize()
        assert np.array_equal(out16.host().view(np.uint16).reshape(h, w, 4), _oracle16(oracle, s, depth, planes, alpha, w, h)), planes
        out16.check(f"convert16 {w}x{h} depth {depth} planes {planes}")


@pytest.mark.gpu
def test_device_conversions_refuse_bad_arguments_and_write_nothing(itw, gpu):
    """-1, and no launch: planes outside 1 .. 4, an empty surface, alpha without its plane (plane 3; plane 2 for 32-bit -> half)."""
    import torch
    L = itw.lib()
    L.itwSetStream(torch.cuda.current_stream().cuda_stream)
    w, h = 16, 4
    d_src = torch.zeros(w * h * 5 * 4, dtype=torch.uint8, device=gpu)
    out = guarded(w * h * 8, device=gpu)
    untouched = out.host().copy()
    s, d = d_src.data_ptr(), out.ptr
    for depth in (8, 16, 32):
        for planes, ww, hh in ((0, w, h), (5, w, h), (-1, w, h), (3, 0, h), (3, w, 0), (3, -4, h), (3, w, -4)):
            assert L.itwConvertToRGBA8Device(s, depth, planes, 0, 0, ww, hh, d) == -1, (depth, planes, ww, hh)
            assert L.itwConvertToRGBA16FDevice(s, depth, planes, 0, ww, hh, d) == -1, (depth, planes, ww, hh)
        for gamma in ((0, 1) if depth == 32 else (0,)):
            assert L.itwConvertToRGBA8Device(s, depth, 3, 1, gamma, w, h, d) == -1, (depth, gamma)          # every route but 32 -> half:
        if depth != 32:
            assert L.itwConvertToRGBA16FDevice(s, depth, 3, 1, w, h, d) == -1, depth                           # alpha is plane 3
    assert L.itwConvertToRGBA16FDevice(s, 32, 2, 1, w, h, d) == -1                                             # 32 -> half: alpha is plane 2
    assert L.itwConvertToRGBA16FDevice(s, 32, 1, 1, w, h, d) == -1
    torch.cuda.synchronize()
    assert np.array_equal(out.host(), untouched)
    out.check("refused conversions")
