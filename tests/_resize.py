"""The free-size chain of include/itw_dispatch.h ("Mip chains: free sizes", ITW_MIP_RESIZE) restated in numpy, one fp32 operation per line:
DirectXTex's _ResizePointFilter, _ResizeBoxFilter, _ResizeLinearFilter, _ResizeCubicFilter and _ResizeTriangleFilter
(DirectXTexResize.cpp:242-780) between any pair of sizes.  Cubic interpolation, the triangle lists, widen and store are
tests/_mip_filters.py's; this file adds the point index, the box at exactly 2:1, _CreateLinearFilter with its wrap branches, bounduvw with
mirror, and the triangle accumulation over a free pair.  tests/golden/resize_ref.npz pins it to the reference's own functions
(tools/make_resize_golden.py); the case list both share is here."""
import numpy as np

import _mip_filters as MF
import _mipgen as M
import _srgb_mips as S

F = np.float32
KINDS = MF.KINDS
FILTERS = ("point", "box", "linear", "cubic", "triangle")
CLAMP, WRAP, MIRROR = 0, 1, 2

# (sizes, seed): two sizes are a resize, more a chain; the table of the issue, in its order
CASES = [(((5, 3), (5, 3)), 61), (((1, 1), (4, 4)), 62), (((4, 4), (1, 1)), 63), (((4, 4), (8, 8)), 64), (((16, 16), (8, 8)), 65),
         (((3, 5), (7, 4)), 66), (((7, 7), (3, 3)), 67), (((64, 64), (16, 16)), 68), (((130, 70), (3, 2)), 69), (((100, 36), (17, 64)), 70),
         (((33, 9), (257, 70)), 71), (((1000, 600), (256, 256)), 72), (((255, 255), (1024, 768)), 73), (((20, 12), (33, 7), (8, 8)), 74)]
# (kind, address) of every recorded per-axis table
TABLE_VARIANTS = (("linear", CLAMP), ("linear", WRAP), ("cubic", CLAMP), ("cubic", WRAP), ("cubic", MIRROR), ("triangle", CLAMP), ("triangle", WRAP))


def sizes_name(sizes):
    return "_".join(f"{w}x{h}" for w, h in sizes)


def case_name(filt, addr, sizes):
    return f"{filt}_{addr or 'clamp'}_{sizes_name(sizes)}"


def table_name(kind, address, source, dest):
    return f"{kind}table_{('clamp', 'wrap', 'mirror')[address]}_{source}_{dest}"


def table_pairs():
    """every (source, dest) pair of an axis of a level pair of CASES, once"""
    pairs = []
    for sizes, _ in CASES:
        for (sw, sh), (dw, dh) in zip(sizes, sizes[1:]):
            for p in ((sw, dw), (sh, dh)):
                if p not in pairs:
                    pairs.append(p)
    return pairs


def linear_wrap_refused(sizes, addr):
    """the refusal of the header: the linear filter with a wrap bit on an axis where dest >= source > 1, at any level pair"""
    return any(("u" in addr and dw >= sw > 1) or ("v" in addr and dh >= sh > 1) for (sw, sh), (dw, dh) in zip(sizes, sizes[1:]))


def variants(sizes):
    """the (filter, address) pairs a case is recorded under: address "" | "u" | "v" | "uv" (wrap) or "mirror" (both axes; cubic only)"""
    out = []
    for filt in FILTERS:
        if filt == "box" and not all(2 * dw == sw and 2 * dh == sh for (sw, sh), (dw, dh) in zip(sizes, sizes[1:])):
            continue
        for addr in MF.WRAPS:
            if filt == "linear" and linear_wrap_refused(sizes, addr):
                continue
            out.append((filt, addr))
        if filt == "cubic":
            out.append((filt, "mirror"))
    return out


def axis_address(addr, axis):
    """the bounduvw case of one axis ("u" or "v") under a case's address"""
    return MIRROR if addr == "mirror" else WRAP if axis in addr else CLAMP


# ---- per-axis tables ----------------------------------------------------------------------------------------------------------------------

def point_index(source, dest):
    """(u * ((source << 16) / dest)) >> 16 in 64-bit integers"""
    step = (source << 16) // dest
    return (np.arange(dest, dtype=np.int64) * step) >> 16


def linear_filter(source, dest, wrap):
    """_CreateLinearFilter as written, wrap branches included: (u0, weight0, u1, weight1)."""
    scale = F(source) / F(dest)
    u = np.arange(dest, dtype=F)
    t = u + F(0.5)
    t = t * scale
    src_b = t + F(0.5)
    isrc_b = src_b.astype(np.int64)
    isrc_a = isrc_b - 1
    isrc_a = np.where(isrc_a < 0, source - 1 if wrap else 0, isrc_a)
    isrc_b = np.where(isrc_b >= source, 0 if wrap else source - 1, isrc_b)
    w = F(1.0) + isrc_b.astype(F)
    weight0 = w - src_b
    weight1 = F(1.0) - weight0
    assert weight0.dtype == F and weight1.dtype == F
    return isrc_a, weight0, isrc_b, weight1


def bound(u, maxu, address):
    """bounduvw: wrap, else mirror, then the clamp."""
    u = np.asarray(u, dtype=np.int64)
    if address == WRAP:
        u = np.where(u < 0, maxu + u + 1, np.where(u > maxu, u - maxu - 1, u))
    elif address == MIRROR:
        u = np.where(u < 0, -u - 1, np.where(u > maxu, maxu - (u - maxu - 1), u))
    return np.maximum(np.minimum(u, maxu), 0)


def cubic_filter(source, dest, address):
    """_CreateCubicFilter under any addressing: ((dest, 4) taps, (dest,) fp32 x); (ptrdiff_t)srcB truncates toward zero."""
    scale = F(source) / F(dest)
    u = np.arange(dest, dtype=F)
    t = u + F(0.5)
    t = t * scale
    src_b = t - F(0.5)
    b = bound(np.trunc(src_b).astype(np.int64), source - 1, address)
    taps = np.stack([bound(b - 1, source - 1, address), b, bound(b + 1, source - 1, address), bound(b + 2, source - 1, address)], axis=1)
    x = src_b - b.astype(F)
    assert x.dtype == F
    return taps, x


# ---- the five filters over widened texels ---------------------------------------------------------------------------------------------------

def point_unrounded(f, dw, dh):
    h, w = f.shape[:2]
    return f[point_index(h, dh)][:, point_index(w, dw)]


def box_unrounded(f, dw, dh):
    h, w = f.shape[:2]
    assert 2 * dw == w and 2 * dh == h
    v = f[0::2, 0::2] + f[1::2, 0::2]
    v = v + f[0::2, 1::2]
    v = v + f[1::2, 1::2]
    return v * F(0.25)


def linear_unrounded(f, dw, dh, wrap_u, wrap_v):
    h, w = f.shape[:2]
    xu0, xw0, xu1, xw1 = linear_filter(w, dw, wrap_u)
    yu0, yw0, yu1, yw1 = linear_filter(h, dh, wrap_v)
    xw0, xw1 = xw0[None, :, None], xw1[None, :, None]
    yw0, yw1 = yw0[:, None, None], yw1[:, None, None]
    r0, r1 = f[yu0], f[yu1]
    with np.errstate(invalid="ignore", over="ignore"):
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


def cubic_unrounded(f, dw, dh, addr_u, addr_v):
    h, w = f.shape[:2]
    tx, xx = cubic_filter(w, dw, addr_u)
    ty, xy = cubic_filter(h, dh, addr_v)
    xx, xy = xx[None, :, None], xy[:, None, None]
    rows = []
    for k in range(4):
        r = f[ty[:, k]]
        rows.append(MF.cubic_interpolate(r[:, tx[:, 0]], r[:, tx[:, 1]], r[:, tx[:, 2]], r[:, tx[:, 3]], xx))
    return MF.cubic_interpolate(rows[0], rows[1], rows[2], rows[3], xy)


def _by_rank(lists, dest):
    """For every destination the entries that reach it in order of arrival (sources ascending, a source's own entries as stored, so one
    source may stand twice): (rank, dest) int64 sources, fp32 weights and a bool mask.  A destination nothing reaches has no rank."""
    per = [[] for _ in range(dest)]
    for u, to in enumerate(lists):
        for d, w in to:
            per[d].append((u, w))
    ranks = max(len(p) for p in per)
    src = np.zeros((ranks, dest), dtype=np.int64)
    wgt = np.zeros((ranks, dest), dtype=F)
    have = np.zeros((ranks, dest), dtype=bool)
    for d, p in enumerate(per):
        for r, (u, w) in enumerate(p):
            src[r, d], wgt[r, d], have[r, d] = u, w, True
    return src, wgt, have


def triangle_unrounded_scatter(f, dw, dh, wrap_u, wrap_v):
    """The accumulation as the reference runs it (:703-730): source rows, source columns, the row's destinations, the column's."""
    h, w = f.shape[:2]
    xl, yl = MF.triangle_lists(w, dw, wrap_u), MF.triangle_lists(h, dh, wrap_v)
    acc = np.zeros((dh, dw, 4), dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        for y in range(h):
            for x in range(w):
                for v, yw in yl[y]:
                    for u, xw in xl[x]:
                        wgt = yw * xw
                        t = f[y, x] * wgt
                        acc[v, u] = t + acc[v, u]
    return acc


def triangle_unrounded(f, dw, dh, wrap_u, wrap_v):
    """The same sums, a row's columns vectorised by their rank of arrival at each destination.  Where one source row reaches one
    destination row twice the order within a texel (row entries outside, column entries inside) is no longer rank order: the scatter."""
    h, w = f.shape[:2]
    xl, yl = MF.triangle_lists(w, dw, wrap_u), MF.triangle_lists(h, dh, wrap_v)
    if any(len({v for v, _ in to}) != len(to) for to in yl):
        return triangle_unrounded_scatter(f, dw, dh, wrap_u, wrap_v)
    src, wgt, have = _by_rank(xl, dw)
    acc = np.zeros((dh, dw, 4), dtype=F)                              # (a destination no entry reaches stays 0)
    with np.errstate(invalid="ignore", over="ignore"):
        for y in range(h):
            row = f[y]
            for v, yw in yl[y]:
                for r in range(src.shape[0]):
                    m = have[r]
                    wv = (yw * wgt[r, m])[:, None]
                    t = row[src[r, m]] * wv
                    acc[v, m] = t + acc[v, m]
    assert acc.dtype == F
    return acc


def pair_filter(filt, sw, sh, dw, dh):
    """the default's choice (_PerformResizeUsingCustomFilters): box at exactly 2:1 on both axes, else linear"""
    if filt is not None:
        return filt
    return "box" if 2 * dw == sw and 2 * dh == sh else "linear"


def store_plain(v, kind):
    """the store of point, box and linear: the kind's own, the raw codes by (uint8_t)min(v + 0.5f, 255.0f)"""
    if kind == "srgb":
        return S.store(v, np.uint8)
    return M.store(v, np.uint16 if kind == "rgba16f" else np.uint8)


def level(src, size, filt=None, addr="", kind=None):
    """`src` (a stored image) resized to size = (w, h) under filt (None: the default) and addr ("" | "u" | "v" | "uv" | "mirror")."""
    kind = kind or ("rgba16f" if src.dtype == np.uint16 else "rgba8")
    dw, dh = size
    sh, sw = src.shape[:2]
    filt = pair_filter(filt, sw, sh, dw, dh)
    f = MF.widen(src, kind)
    wrap_u, wrap_v = addr != "mirror" and "u" in addr, addr != "mirror" and "v" in addr
    if filt == "point":
        out = store_plain(point_unrounded(f, dw, dh), kind)
    elif filt == "box":
        out = store_plain(box_unrounded(f, dw, dh), kind)
    elif filt == "linear":
        out = store_plain(linear_unrounded(f, dw, dh, wrap_u, wrap_v), kind)
    elif filt == "cubic":
        out = MF.store(cubic_unrounded(f, dw, dh, axis_address(addr, "u"), axis_address(addr, "v")), kind)
    else:
        assert filt == "triangle"
        out = MF.store(triangle_unrounded(f, dw, dh, wrap_u, wrap_v), kind)
    return np.ascontiguousarray(out)


def chain(base, sizes, filt=None, addr="", kind=None):
    """[base, level 1, ...]: level l of size sizes[l] from level l-1 as stored (sizes[0] is the base's)."""
    out = [np.ascontiguousarray(base)]
    for size in sizes[1:]:
        out.append(level(out[-1], size, filt, addr, kind))
    return out
