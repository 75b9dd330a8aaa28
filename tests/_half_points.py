"""Where a float -> half conversion can round wrongly, as float bit patterns (tests/test_prepass_convert.py, tests/test_reference_pins.py).

The pin is IEEE 754 round to nearest even (oracle/prepass.c).  A rounding rule can only go wrong next to a decision
point, and those are the half values themselves and the midpoints between neighbouring halves: `structured()` holds each of them +-3
floats.  `legacy_half_bits` is the rule the checker used to restate (the 2012-2015 DirectXMath software path: sticky bits of a half
denormal dropped, everything above 65504 sent to inf); it is here only to show that the point sets tell the two rules apart."""
import numpy as np

SIGN = np.uint32(0x80000000)
DENORMAL_RANGE = (0x33000000 - 16, 0x38800000 + 16)      # 2^-25 .. 2^-14: every float a half denormal (or the 0 / 2^-24 decision) takes
TOP_RANGE = (0x477f0000, 0x47800010)                     # 65280 .. just past 65536: the last finite halves, 65504, 65520, the way to inf
STRUCTURED_PER_SIGN = 444_413
LEGACY_DIFFERS_PER_SIGN = (6_144, 4_095)                 # floats at which the legacy rule is not IEEE: in DENORMAL_RANGE, in TOP_RANGE
LEGACY_DIFFERS_STRUCTURED = (1_024, 6)                   # ... and how many of them structured() holds


def structured():
    """Every finite non-negative half, and every midpoint between two neighbouring halves (65520 = the midpoint towards 2^16 included),
    each with the three floats below and above it: 444 413 non-negative float bit patterns, increasing."""
    halves = np.arange(0x7c00, dtype=np.uint16).view(np.float16).astype(np.float64)
    upper = np.append(halves[1:], 65536.0)
    mids = (halves + upper) / 2                                                    # exact in double, and every one of them is a float
    centre = np.concatenate([halves, mids]).astype(np.float32)
    assert np.array_equal(centre.astype(np.float64), np.concatenate([halves, mids]))
    bits = centre.view(np.uint32).astype(np.int64)[:, None] + np.arange(-3, 4)[None, :]
    bits = np.unique(bits[bits >= 0])
    assert bits.size == STRUCTURED_PER_SIGN and bits[-1] < 0x7f800000
    return bits.astype(np.uint32)


def both_signs(bits):
    return np.concatenate([bits, bits | SIGN])


def whole_range(lo_hi, stride=1, start=0):
    lo, hi = lo_hi
    return np.arange(lo + start, hi, stride, dtype=np.int64).astype(np.uint32)


def ieee_half_bits(bits):
    """numpy's float32 -> float16: IEEE round to nearest even."""
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32).astype(np.float16).view(np.uint16)


def legacy_half_bits(bits):
    """The rule oracle/prepass.c restated before it was corrected (finite inputs and inf; NaN not modelled)."""
    b = np.asarray(bits, dtype=np.uint32).astype(np.uint64)
    sign = (b & 0x80000000) >> np.uint64(16)
    x = b & 0x7fffffff
    shift = np.minimum(np.uint64(113) - np.minimum(x >> np.uint64(23), np.uint64(113)), np.uint64(63))
    den = np.where(shift < 32, (np.uint64(0x800000) | (x & 0x7fffff)) >> shift, 0).astype(np.uint64)
    y = np.where(x < 0x38800000, den, (x + 0xc8000000) & 0xffffffff).astype(np.uint64)
    r = ((y + 0x0fff + ((y >> np.uint64(13)) & 1)) >> np.uint64(13)) & 0x7fff
    r = np.where(x > 0x477fe000, 0x7c00, r).astype(np.uint64)
    return (r | sign).astype(np.uint16)
