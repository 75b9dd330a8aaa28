"""The sRGB colour kind of the mip filters (include/itw_dispatch.h, "Mip chains", ITW_MIP_SRGB) restated in numpy: the two tables recomputed
here with `decimal` -- not read from csrc/srgb_tables.h, which tests/test_srgb_mips_cpu.py compares with them -- and tests/_mipgen.py's box
and linear models with this kind's widen and store in the places of the plain ones.  Images are (H, W, 4) uint8: R, G, B sRGB coded, A linear.
"""
import decimal
from fractions import Fraction

import numpy as np

import _mipgen as M

F = np.float32
D = decimal.Decimal


def srgb_to_linear_exact(x):
    """f of IEC 61966-2-1 for a Decimal code value in [0, 1], under the caller's decimal context."""
    if x <= D("0.04045"):
        return x / D("12.92")
    return ((x + D("0.055")) / D("1.055")) ** D("2.4")


def nearest_fp32(x):
    """The fp32 nearest to the Decimal x >= 0: of the float32 of its double and that value's two neighbours, the one closest as an exact
    fraction (a tie would be ambiguous: there is none)."""
    exact = Fraction(x)
    mid = F(float(x))
    cands = {mid, np.nextafter(mid, F(np.inf)), np.nextafter(mid, F(-np.inf))}
    ranked = sorted((abs(Fraction(float(c)) - exact), float(c)) for c in cands if c >= 0)
    assert len(ranked) == 1 or ranked[0][0] < ranked[1][0], x
    return F(ranked[0][1])


def _tables():
    with decimal.localcontext() as ctx:
        ctx.prec = 80
        dec = np.array([nearest_fp32(srgb_to_linear_exact(D(c) / D(255))) for c in range(256)], dtype=F)
        thr = np.array([F(0)] + [nearest_fp32(srgb_to_linear_exact((D(k) - D("0.5")) / D(255))) for k in range(1, 256)], dtype=F)
    return dec, thr


DECODE, THR = _tables()              # D[c], c = 0..255; T[k], k = 1..255 (THR[0] is not part of the definition)


def encode(v):
    """E(v): the number of k in 1..255 with v >= T[k], for an fp32 array."""
    v = np.asarray(v, dtype=F)
    return np.searchsorted(THR[1:], v, side="right").astype(np.uint8)


def encode_by_counting(v):
    """The definition as written, for a handful of values (256 compares each)."""
    v = np.asarray(v, dtype=F)
    return (v[..., None] >= THR[1:]).sum(axis=-1).astype(np.uint8)


def widen(img):
    assert img.dtype == np.uint8 and img.shape[-1] == 4
    out = np.empty(img.shape, dtype=F)
    out[..., :3] = DECODE[img[..., :3]]
    out[..., 3] = img[..., 3].astype(F)
    return out


def store(v, dtype):
    assert dtype == np.uint8 and v.dtype == F
    out = np.empty(v.shape, dtype=np.uint8)
    out[..., :3] = encode(v[..., :3])
    out[..., 3] = M.store_rgba8(v[..., 3])
    return out


def _swapped(step, src):
    """tests/_mipgen.py's `step` with this kind's widen and store swapped in for the call."""
    saved = M.widen, M.store
    M.widen, M.store = widen, store
    try:
        return step(src)
    finally:
        M.widen, M.store = saved


def box_level(src):
    return _swapped(M.box_level, src)


def linear_level(src):
    return _swapped(M.linear_level, src)


def chain(base, levels=0):
    """[base, level 1, ...] as M.chain makes it: box for a power-of-two base, else linear; level l from level l-1 as stored."""
    h, w = base.shape[:2]
    n = levels or M.levels_of(w, h)
    step = box_level if M.is_pow2(w) and M.is_pow2(h) else linear_level
    out = [np.ascontiguousarray(base)]
    for _ in range(1, n):
        out.append(np.ascontiguousarray(step(out[-1])))
    return out


def threshold_neighbourhood(radius=3):
    """Every T[k] and `radius` floats either side, +-0, the smallest denormal, 1.0 and the next float up, 1.5: where an encode can go wrong."""
    bits = THR[1:].view(np.uint32).astype(np.int64)
    near = (bits[:, None] + np.arange(-radius, radius + 1)[None, :]).reshape(-1).astype(np.uint32).view(F)
    extra = np.array([0.0, -0.0, np.float32(1e-45), 1.0, np.nextafter(F(1), F(2)), 1.5], dtype=F)
    return np.concatenate([near, extra])
