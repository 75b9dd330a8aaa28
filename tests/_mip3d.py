"""The volume mip filters of include/itw_dispatch.h ("Mip chains: volumes") restated in numpy, one fp32 operation per line: DirectXTex's
_Generate3DMipsPointFilter, _BoxFilter, _LinearFilter, _CubicFilter and _TriangleFilter (DirectXTexMipmaps.cpp:1371-2497) over the per-axis
tables of tests/_mipgen.py, tests/_mip_filters.py and tests/_resize.py, for the three texel kinds.  A volume is a (D, H, W, 4) array: uint8
codes, or uint16 half bits.  Once the depth is 1 every filter is the reference's 2D branch: the same expression over the one slice.

tests/golden/mip3d_ref.npz pins this model to the reference's own functions (tools/make_mip3d_golden.py); the one stated divergence -- a
box level whose source height is 1 while its width is not takes row 2y+1 = row 2y, where the reference reads a stale scanline -- is
outside the recorded levels."""
import numpy as np

import _mipgen as M
import _mip_filters as MF
import _resize as R

F = np.float32
KINDS = MF.KINDS
FILTERS = ("box", "point", "linear", "cubic", "triangle")
WRAPS = ("", "w", "uvw")                                    # what the cubic and triangle cases are recorded under

# (width, height, depth, seed): recorded whole under every filter
CASES = [(2, 2, 2, 71), (4, 4, 4, 72), (8, 8, 8, 73), (4, 8, 2, 74), (2, 4, 8, 75), (4, 16, 4, 76), (1, 1, 8, 77), (1, 8, 1, 78), (16, 16, 16, 79),
         (5, 3, 7, 80), (7, 7, 7, 81), (3, 12, 5, 82), (12, 20, 6, 83), (8, 8, 1, 84), (12, 20, 1, 85)]
SHA_CASES = [(32, 32, 32, 86), (32, 64, 16, 87), (33, 20, 17, 88)]          # as SHA-256 only
WIDE_BOX_CASES = [(8, 2, 4, 89), (16, 4, 16, 90)]                            # box only; the levels whose source height is >= 2


def levels_of(w, h, d):
    """1 + floor(log2(max(w, h, d))); 0 for a size below 1."""
    if w < 1 or h < 1 or d < 1:
        return 0
    n, m = 1, max(w, h, d)
    while m > 1:
        m >>= 1
        n += 1
    return n


def level_size(w, h, d, l):
    return max(1, w >> l), max(1, h >> l), max(1, d >> l)


def slices_of(d, levels):
    return sum(max(1, d >> l) for l in range(levels))


def default_filter(w, h, d):
    """GenerateMipMaps3D's default: box when all three sizes are powers of two, triangle otherwise."""
    return "box" if M.is_pow2(w) and M.is_pow2(h) and M.is_pow2(d) else "triangle"


def recorded_levels(filt, w, h, d):
    """The levels of a case that the recording holds: all of them, but for the box filter those whose source height is 1 while its width
    is not (the stale-scanline levels)."""
    out = []
    for l in range(1, levels_of(w, h, d)):
        sw, sh, _ = level_size(w, h, d, l - 1)
        if filt == "box" and sh == 1 and sw > 1:
            break
        out.append(l)
    return out


def case_name(filt, wrap, w, h, d):
    return f"{filt}_{wrap or 'clamp'}_{w}x{h}x{d}"


def variants(w, h, d):
    """(filter, wrap) pairs a case is recorded under"""
    out = [("point", ""), ("linear", "")]
    if default_filter(w, h, d) == "box":
        out.insert(0, ("box", ""))
    for filt in ("cubic", "triangle"):
        out += [(filt, wrap) for wrap in WRAPS]
    return out


# ---- the five filters over widened texels (D, H, W, 4) ----------------------------------------------------------------------------------

def _box_taps(f):
    """the four taps of every slice in AVERAGE4's order; an axis of size 1 gives the second tap = the first"""
    _, h, w = f.shape[:3]
    r0, r1 = (f[:, 0::2], f[:, 1::2]) if h > 1 else (f, f)
    c0, c1 = (slice(0, None, 2), slice(1, None, 2)) if w > 1 else (slice(None), slice(None))
    return r0[:, :, c0], r1[:, :, c0], r0[:, :, c1], r1[:, :, c1]


def box_unrounded(f):
    d = f.shape[0]
    p = _box_taps(f)
    with np.errstate(invalid="ignore", over="ignore"):
        if d > 1:
            a, b = [t[0::2] for t in p], [t[1::2] for t in p]
            v = a[0] + a[1]
            v = v + a[2]
            v = v + a[3]
            v = v + b[0]
            v = v + b[1]
            v = v + b[2]
            v = v + b[3]
            return v * F(0.125)
        v = p[0] + p[1]
        v = v + p[2]
        v = v + p[3]
        return v * F(0.25)


def point_unrounded(f):
    d, h, w = f.shape[:3]
    nw, nh, nd = level_size(w, h, d, 1)
    return f[R.point_index(d, nd)][:, R.point_index(h, nh)][:, :, R.point_index(w, nw)]


def linear_unrounded(f):
    d, h, w = f.shape[:3]
    nw, nh, nd = level_size(w, h, d, 1)
    planes = np.stack([R.linear_unrounded(f[z], nw, nh, False, False) for z in range(d)])
    if d == 1:
        return planes
    zu0, zw0, zu1, zw1 = R.linear_filter(d, nd, False)
    with np.errstate(invalid="ignore", over="ignore"):
        a = zw0[:, None, None, None] * planes[zu0]
        b = zw1[:, None, None, None] * planes[zu1]
        v = a + b
    assert v.dtype == F
    return v


def cubic_unrounded(f, wrap):
    d, h, w = f.shape[:3]
    nw, nh, nd = level_size(w, h, d, 1)
    au, av, aw = (R.WRAP if c in wrap else R.CLAMP for c in "uvw")
    planes = np.stack([R.cubic_unrounded(f[z], nw, nh, au, av) for z in range(d)])
    if d == 1:
        return planes
    tz, xz = R.cubic_filter(d, nd, aw)
    return MF.cubic_interpolate(planes[tz[:, 0]], planes[tz[:, 1]], planes[tz[:, 2]], planes[tz[:, 3]], xz[:, None, None, None])


def triangle_unrounded_scatter(f, wrap):
    """The accumulation as the reference runs it (:2338-2428): source slices, rows, texels; the slice's destinations, the row's, the texel's."""
    d, h, w = f.shape[:3]
    nw, nh, nd = level_size(w, h, d, 1)
    xl, yl, zl = MF.triangle_lists(w, nw, "u" in wrap), MF.triangle_lists(h, nh, "v" in wrap), MF.triangle_lists(d, nd, "w" in wrap)
    acc = np.zeros((nd, nh, nw, 4), dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        for z in range(d):
            for y in range(h):
                for x in range(w):
                    for s, zw in zl[z]:
                        for v, yw in yl[y]:
                            for u, xw in xl[x]:
                                wgt = zw * yw
                                wgt = wgt * xw
                                t = f[z, y, x] * wgt
                                acc[s, v, u] = t + acc[s, v, u]
    return acc


def triangle_unrounded(f, wrap):
    """The same sums, a row's texels vectorised by their rank of arrival at each destination.  Where one source slice or row reaches one
    destination twice the order within a texel is no longer rank order: the scatter."""
    d, h, w = f.shape[:3]
    nw, nh, nd = level_size(w, h, d, 1)
    xl, yl, zl = MF.triangle_lists(w, nw, "u" in wrap), MF.triangle_lists(h, nh, "v" in wrap), MF.triangle_lists(d, nd, "w" in wrap)
    if any(len({v for v, _ in to}) != len(to) for lists in (yl, zl) for to in lists):
        return triangle_unrounded_scatter(f, wrap)
    src, wgt, have = R._by_rank(xl, nw)
    acc = np.zeros((nd, nh, nw, 4), dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        for z in range(d):
            for y in range(h):
                row = f[z, y]
                for s, zw in zl[z]:
                    for v, yw in yl[y]:
                        zy = zw * yw
                        for r in range(src.shape[0]):
                            m = have[r]
                            wv = (zy * wgt[r, m])[:, None]
                            t = row[src[r, m]] * wv
                            acc[s, v, m] = t + acc[s, v, m]
    assert acc.dtype == F
    return acc


def level(src, filt=None, wrap="", kind=None):
    """The next level of the stored volume `src` (D, H, W, 4) under filt (None: the default of src's own size) and wrap (letters of "uvw")."""
    kind = kind or ("rgba16f" if src.dtype == np.uint16 else "rgba8")
    d, h, w = src.shape[:3]
    filt = filt or default_filter(w, h, d)
    f = MF.widen(src, kind)
    if filt == "box":
        out = R.store_plain(box_unrounded(f), kind)
    elif filt == "point":
        out = R.store_plain(point_unrounded(f), kind)
    elif filt == "linear":
        out = R.store_plain(linear_unrounded(f), kind)
    elif filt == "cubic":
        out = MF.store(cubic_unrounded(f, wrap), kind)
    else:
        assert filt == "triangle"
        out = MF.store(triangle_unrounded(f, wrap), kind)
    return np.ascontiguousarray(out)


def chain(base, filt=None, wrap="", kind=None, levels=0):
    """[base, level 1, ...]: the filter (None: the default, chosen once from the base) on every level, level l from level l-1 as stored."""
    d, h, w = base.shape[:3]
    filt = filt or default_filter(w, h, d)
    out = [np.ascontiguousarray(base)]
    for _ in range(1, levels or levels_of(w, h, d)):
        out.append(level(out[-1], filt, wrap, kind))
    return out


def seeded_half_volume(d, h, w, seed):
    return MF.seeded_half_image(d * h, w, seed).reshape(d, h, w, 4)


def seeded_byte_volume(d, h, w, seed):
    return MF.seeded_byte_image(d * h, w, seed).reshape(d, h, w, 4)
