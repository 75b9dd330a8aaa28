"""The two mip rules for cut-out RGBA8 textures (include/itw_dispatch.h, "Mip chains of cut-out textures") restated in numpy on top of
tests/_mipgen.py and tests/_srgb_mips.py: A, alpha-weighted colour, one fp32 operation per line, with the integer form of the raw-code box
beside it; B, coverage kept per level, in Python integers.  Images are (H, W, 4) uint8.  A report row is the tuple
(texels, covered_plain, covered, threshold) of struct itw_mip_coverage."""
import numpy as np

import _mipgen as M
import _srgb_mips as S

F = np.float32


# ---- the two filters over widened fp32 texels, unrounded: the expressions of tests/_mipgen.py box_level / linear_level --------------------

def box_filter(f):
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
    assert v.dtype == F
    return v


def linear_filter(f):
    h, w = f.shape[:2]
    nw, nh = max(1, w >> 1), max(1, h >> 1)
    xu0, xw0, xu1, xw1 = M.linear_filter(w, nw)
    yu0, yw0, yu1, yw1 = M.linear_filter(h, nh)
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
    return v


# ---- A: alpha-weighted colour --------------------------------------------------------------------------------------------------------------

def weighted_unrounded(src, srgb, linear):
    """(the texel before the store, the mask of texels whose filtered alpha is not above 0) of one weighted level."""
    filt = linear_filter if linear else box_filter
    f = S.widen(src) if srgb else M.widen(src)
    a = f[..., 3:4]
    p = f.copy()
    p[..., :3] = f[..., :3] * a                                   # p = c * a, one multiply per tap
    vp = filt(p)                                                  # P[k], and va in channel 3
    plain = filt(f)
    va = vp[..., 3:4]
    with np.errstate(divide="ignore", invalid="ignore"):
        col = vp[..., :3] / va                                    # one correctly rounded fp32 division
    out = plain.copy()                                            # alpha is the plain rule's: the same expression over the same values
    assert np.array_equal(plain[..., 3], vp[..., 3])
    out[..., :3] = np.where(va > 0, col, plain[..., :3])
    assert out.dtype == F
    return out, ~(va[..., 0] > 0)


def weighted_level(src, srgb=False, linear=False):
    v, _ = weighted_unrounded(src, srgb, linear)
    return (S.store if srgb else M.store)(v, np.uint8)


def invisible_mask(src, linear=False):
    """The output texels of the level filtered from `src` whose va is not above 0: they take the plain rule's colour."""
    return weighted_unrounded(src, False, linear)[1]


def box_level_weighted_integer(src):
    """The weighted box on raw codes as the integer rule it equals: (2 * sum(a c) + sum(a)) // (2 * sum(a)); sum(a) == 0: the plain rule."""
    s = src.astype(np.int64)
    h, w = s.shape[:2]
    r0, r1 = (s[0::2], s[1::2]) if h > 1 else (s, s)
    c0, c1 = (slice(0, None, 2), slice(1, None, 2)) if w > 1 else (slice(None), slice(None))
    taps = [r0[:, c0], r1[:, c0], r0[:, c1], r1[:, c1]]
    sa = sum(t[..., 3] for t in taps)
    out = np.empty(taps[0].shape, dtype=np.uint8)
    for k in range(3):
        sac = sum(t[..., 3] * t[..., k] for t in taps)
        plain = (sum(t[..., k] for t in taps) + 2) >> 2
        out[..., k] = np.where(sa > 0, (2 * sac + sa) // np.maximum(2 * sa, 1), plain)
    out[..., 3] = (sa + 2) >> 2
    return out


def weighted_ratio_fp32(num, den):
    """What the device computes for the raw-code box from sum(a c) = num and sum(a) = den > 0 (int arrays): the four-tap sums are exact in
    fp32 and so is * 0.25f; one division; the RGBA8 store."""
    p = num.astype(F) * F(0.25)
    va = den.astype(F) * F(0.25)
    v = p / va
    return M.store_rgba8(v)


def weighted_ratio_integer(num, den):
    return ((2 * num + den) // (2 * den)).astype(np.uint8)


# ---- B: coverage ---------------------------------------------------------------------------------------------------------------------------

def histogram(alpha):
    return np.bincount(np.asarray(alpha, dtype=np.uint8).reshape(-1), minlength=256).astype(np.int64)


def ge_counts(hist):
    """ge[t]: the texels with a >= t, t = 0 .. 255."""
    return [int(v) for v in np.cumsum(np.asarray(hist, dtype=np.int64)[::-1])[::-1]]


def target(cov0, n, n0):
    return (int(cov0) * int(n) + int(n0) // 2) // int(n0)


def threshold(hist, k, r):
    """t*: the t in 1 .. 255 minimising (|ge[t] - K|, |t - r|, t), by brute force over the triple."""
    ge = ge_counts(hist)
    return min(range(1, 256), key=lambda t: (abs(ge[t] - k), abs(t - r), t))


def rescale(alpha, r, t):
    a = np.asarray(alpha).astype(np.int64)
    return np.minimum(255, (a * int(r)) // int(t)).astype(np.uint8)


def apply_coverage(levels, r):
    """`levels` of one item as generated, coverage off -> (levels with the alpha of every level >= 1 replaced, report rows)."""
    a0 = levels[0][..., 3]
    n0, cov0 = a0.size, int(np.count_nonzero(a0 >= r))
    out, rows = [levels[0]], [(n0, cov0, cov0, r)]
    for lv in levels[1:]:
        a = lv[..., 3]
        hist = histogram(a)
        ge = ge_counts(hist)
        t = threshold(hist, target(cov0, a.size, n0), r)
        new = lv.copy()
        new[..., 3] = rescale(a, r, t)
        out.append(new)
        rows.append((a.size, ge[r], ge[t], t))
    return out, rows


def chain(base, levels=0, srgb=False, weight=False, ref=0):
    """([base, level 1, ...], report rows or None) of one item: box for a power-of-two base, else linear; level l from level l-1 as stored;
    coverage over the whole chain as generated."""
    h, w = base.shape[:2]
    n = levels or M.levels_of(w, h)
    linear = not (M.is_pow2(w) and M.is_pow2(h))
    if weight:
        step = lambda src: weighted_level(src, srgb, linear)
    elif srgb:
        step = S.linear_level if linear else S.box_level
    else:
        step = M.linear_level if linear else M.box_level
    out = [np.ascontiguousarray(base)]
    for _ in range(1, n):
        out.append(np.ascontiguousarray(step(out[-1])))
    if not ref:
        return out, None
    return apply_coverage(out, ref)


# ---- content -------------------------------------------------------------------------------------------------------------------------------

def cutout(h, w, seed, hole=True):
    """Cut-out content: alpha spiked at 0 and 255 with soft edges a few codes wide, arbitrary colour everywhere -- under alpha 0 too.  With
    `hole` the left half (the top half of a one-column image) is fully transparent, so output texels with va == 0 exist down to the level
    that is two texels across."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    field = np.zeros((h, w))
    for _ in range(4):
        fx, fy = rng.uniform(0.05, 0.6, 2)
        field += np.sin(x * fx + rng.uniform(0, 6.28)) * np.sin(y * fy + rng.uniform(0, 6.28))
    alpha = np.clip(field * 400.0 + 100.0, 0, 255).astype(np.uint8)
    if hole:
        if w > 1:
            alpha[:, : w // 2] = 0
        else:
            alpha[: h // 2] = 0
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = alpha
    return img


def noise(h, w, seed):
    """Uniform-noise alpha and colour."""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
