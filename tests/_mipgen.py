"""The mip filters of include/itw_dispatch.h ("Mip chains") restated in numpy, one fp32 operation per line: DirectXTex's non-WIC box and
linear 2D filters (DirectXTexMipmaps.cpp:715-805, :809-917; Filters.h:33-39, :66-106), the RGBA16F scanline store
(DirectXTexConvert.cpp:1634-1646) and the library's own RGBA8 store.  Images are (H, W, 4) arrays: uint8 codes, or uint16 half bits.

tests/golden/mipgen_ref.npz pins this model to the reference's own functions (tools/make_mipgen_golden.py); the one stated divergence --
a box level whose source height is 1 takes row 2y+1 = row 2y, where the reference reads a stale scanline -- is outside the pinned cases.
"""
import numpy as np

F = np.float32


def levels_of(w, h):
    """_CountMips: 1 + floor(log2(max(w, h))); 0 for a size below 1."""
    if w < 1 or h < 1:
        return 0
    n, m = 1, max(w, h)
    while m > 1:
        m >>= 1
        n += 1
    return n


def level_size(w, h, l):
    return max(1, w >> l), max(1, h >> l)


def is_pow2(v):
    return v > 0 and (v & (v - 1)) == 0


def widen(img):
    """A stored image as fp32: the raw codes 0..255, or the halves widened exactly."""
    if img.dtype == np.uint8:
        return img.astype(F)
    assert img.dtype == np.uint16
    return img.view(np.float16).astype(F)


def store_rgba8(v):
    t = v + F(0.5)
    t = np.minimum(t, F(255.0))
    return t.astype(np.uint8)                                     # truncation; v is never negative here


def store_rgba16f(v):
    """Clamp to [-65504, 65504], round to nearest even (numpy's float32 -> float16 is IEEE); a NaN stores 0x7E00."""
    nan = np.isnan(v)
    c = np.maximum(np.where(nan, F(0), v), F(-65504.0))
    c = np.minimum(c, F(65504.0))
    bits = c.astype(np.float16).view(np.uint16).copy()
    bits[nan] = 0x7E00
    return bits


def store(v, dtype):
    return store_rgba8(v) if dtype == np.uint8 else store_rgba16f(v)


def box_level(src):
    """AVERAGE4 over a stored level; a source height (width) of 1 repeats the row (column)."""
    f = widen(src)
    h, w = f.shape[:2]
    r0 = f[0::2] if h > 1 else f
    r1 = f[1::2] if h > 1 else f
    c0 = slice(0, None, 2) if w > 1 else slice(None)
    c1 = slice(1, None, 2) if w > 1 else slice(None)
    p0, p1, p2, p3 = r0[:, c0], r1[:, c0], r0[:, c1], r1[:, c1]
    v = p0 + p1
    v = v + p2
    v = v + p3
    v = v * F(0.25)
    return store(v, src.dtype)


def linear_filter(source, dest):
    """_CreateLinearFilter with clamp addressing: (u0, weight0, u1, weight1) arrays of `dest` entries."""
    scale = F(source) / F(dest)
    u = np.arange(dest, dtype=F)
    t = u + F(0.5)
    t = t * scale
    src_b = t + F(0.5)
    isrc_b = src_b.astype(np.int64)
    isrc_a = np.maximum(isrc_b - 1, 0)
    isrc_b = np.minimum(isrc_b, source - 1)
    w = F(1.0) + isrc_b.astype(F)
    weight0 = w - src_b
    weight1 = F(1.0) - weight0
    assert weight0.dtype == F and weight1.dtype == F
    return isrc_a, weight0, isrc_b, weight1


def linear_level(src):
    f = widen(src)
    h, w = f.shape[:2]
    nw, nh = max(1, w >> 1), max(1, h >> 1)
    xu0, xw0, xu1, xw1 = linear_filter(w, nw)
    yu0, yw0, yu1, yw1 = linear_filter(h, nh)
    xw0, xw1 = xw0[None, :, None], xw1[None, :, None]
    yw0, yw1 = yw0[:, None, None], yw1[:, None, None]
    r0, r1 = f[yu0], f[yu1]
    a = r0[:, xu0] * xw0
    b = r0[:, xu1] * xw1
    top = a + b
    a = r1[:, xu0] * xw0
    b = r1[:, xu1] * xw1
    bot = a + b
    top = yw0 * top
    bot = yw1 * bot
    v = top + bot
    assert v.dtype == F
    return store(v, src.dtype)


def chain(base, levels=0):
    """[base, level 1, ...]: box when width and height are powers of two, else linear; the choice is made once, from the base."""
    h, w = base.shape[:2]
    n = levels or levels_of(w, h)
    step = box_level if is_pow2(w) and is_pow2(h) else linear_level
    out = [np.ascontiguousarray(base)]
    for _ in range(1, n):
        out.append(np.ascontiguousarray(step(out[-1])))
    return out


def box_level_rgba8_integer(src):
    """The box filter on RGBA8 as the integer rule it equals: (a + b + c + d + 2) >> 2."""
    s = src.astype(np.uint32)
    h, w = s.shape[:2]
    r0, r1 = (s[0::2], s[1::2]) if h > 1 else (s, s)
    c0, c1 = (slice(0, None, 2), slice(1, None, 2)) if w > 1 else (slice(None), slice(None))
    return ((r0[:, c0] + r1[:, c0] + r0[:, c1] + r1[:, c1] + 2) >> 2).astype(np.uint8)


def seeded_half_image(h, w, seed):
    """Finite RGBA16F content for the golden cases and the GPU tests: a smooth ramp plus noise, a few large magnitudes and both signs."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0.0, 1.0, (h, w, 4)).astype(F)
    v = v * np.exp2(rng.integers(-12, 12, (h, w, 4))).astype(F)
    bits = v.astype(np.float16).view(np.uint16).copy()
    bits[(bits & 0x7C00) == 0x7C00] = 0x7BFF                      # finite only
    return bits
