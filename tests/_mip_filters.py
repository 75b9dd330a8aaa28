"""The cubic and triangle mip filters of include/itw_dispatch.h ("Mip chains: cubic and triangle") restated in numpy, one fp32 operation
per line: DirectXTex's _Generate2DMipsCubicFilter and _Generate2DMipsTriangleFilter (DirectXTexMipmaps.cpp:921-1103, :1107-1313) over
_CreateCubicFilter, bounduvw, CUBIC_INTERPOLATE and TriangleFilter::_Create (Filters.h:123-205, :249-418), with wrap addressing per axis.
Loads and stores are the texel kinds' of tests/_mipgen.py and tests/_srgb_mips.py; the raw-code store takes its signed form.

tests/golden/mipfilter_ref.npz pins this model to the reference's own functions (tools/make_mipfilter_golden.py).  The cubic filter is
vectorised.  The triangle filter is here twice: triangle_unrounded_scatter is the reference's loop nest as written, texel by texel; and
triangle_unrounded keeps its scatter over source rows and vectorises a row's columns by their rank of arrival at each destination."""
import numpy as np

import _mipgen as M
import _srgb_mips as S

F = np.float32
KINDS = ("rgba16f", "rgba8", "srgb")
WRAPS = ("", "u", "v", "uv")
TF_EPSILON = F(0.00001)


def bound(u, maxu, wrap):
    """bounduvw with mirror off, for an int64 array."""
    u = np.asarray(u, dtype=np.int64)
    if wrap:
        u = np.where(u < 0, maxu + u + 1, np.where(u > maxu, u - maxu - 1, u))
    return np.maximum(np.minimum(u, maxu), 0)


def cubic_filter(source, dest, wrap):
    """_CreateCubicFilter: ((dest, 4) int64 taps, (dest,) fp32 x)."""
    scale = F(source) / F(dest)
    u = np.arange(dest, dtype=F)
    t = u + F(0.5)
    t = t * scale
    src_b = t - F(0.5)
    b = bound(src_b.astype(np.int64), source - 1, wrap)
    taps = np.stack([bound(b - 1, source - 1, wrap), b, bound(b + 1, source - 1, wrap), bound(b + 2, source - 1, wrap)], axis=1)
    x = src_b - b.astype(F)
    assert x.dtype == F
    return taps, x


def cubic_interpolate(p0, p1, p2, p3, x):
    third, sixth, half = F(1.0) / F(3.0), F(1.0) / F(6.0), F(0.5)
    with np.errstate(invalid="ignore", over="ignore"):
        a0 = p1
        d0 = p0 - a0
        d2 = p2 - a0
        d3 = p3 - a0
        a1 = third * d0
        a1 = d2 - a1
        t = sixth * d3
        a1 = a1 - t
        a2 = half * d0
        t = half * d2
        a2 = a2 + t
        a3 = sixth * d3
        t = sixth * d0
        a3 = a3 - t
        t = half * d2
        a3 = a3 - t
        x2 = x * x
        x3 = x2 * x
        r = a1 * x
        r = a0 + r
        t = a2 * x2
        r = r + t
        t = a3 * x3
        r = r + t
    assert r.dtype == F
    return r


def cubic_unrounded(f, wrap_u, wrap_v):
    h, w = f.shape[:2]
    nw, nh = max(1, w >> 1), max(1, h >> 1)
    tx, xx = cubic_filter(w, nw, wrap_u)
    ty, xy = cubic_filter(h, nh, wrap_v)
    xx, xy = xx[None, :, None], xy[:, None, None]
    rows = []
    for k in range(4):
        r = f[ty[:, k]]
        rows.append(cubic_interpolate(r[:, tx[:, 0]], r[:, tx[:, 1]], r[:, tx[:, 2]], r[:, tx[:, 3]], xx))
    return cubic_interpolate(rows[0], rows[1], rows[2], rows[3], xy)


def triangle_lists(source, dest, wrap):
    """TriangleFilter::_Create: per source index the list of (destination, fp32 weight), in the order the reference stores them."""
    scale = F(dest) / F(source)
    scale_inv = F(0.5) / scale
    out = []
    accum_u, accum_w = 0, F(0)
    fdest, fsource = F(dest), F(source)
    for u in range(source):
        to = []
        for j in range(2):
            src = F(u + j) - F(0.5)
            dest_min = src * scale
            dest_max = dest_min + scale
            if not wrap:
                if dest_min < F(0):
                    dest_min = F(0)
                if dest_max > fdest:
                    dest_max = fdest
            k = int(np.floor(dest_min))
            while F(k) < dest_max:
                d0 = F(k)
                d1 = d0 + F(1)
                u0 = k + dest if k < 0 else k - dest if k >= dest else k
                if u0 != accum_u:
                    if accum_w > TF_EPSILON:
                        to.append((accum_u, accum_w))
                    accum_w = F(0)
                    accum_u = u0
                if d0 < dest_min:
                    d0 = dest_min
                if d1 > dest_max:
                    d1 = dest_max
                if not wrap and src < F(0):
                    weight = F(1)
                elif not wrap and (src + F(1)) >= fsource:
                    weight = F(0)
                else:
                    weight = (d0 + d1) * scale_inv
                    weight = weight - src
                span = d1 - d0
                part = span * ((F(1) - weight) if j else weight)
                accum_w = accum_w + part
                assert type(accum_w) is F
                k += 1
        if accum_w > TF_EPSILON:
            to.append((accum_u, accum_w))
        accum_w = F(0)
        out.append(to)
    return out


def triangle_table(source, dest, wrap):
    """The lists flattened as the recording and the library's test hook hold them: (E, 2) int32 of (source, destination), (E,) fp32."""
    lists = triangle_lists(source, dest, wrap)
    idx = np.array([(u, d) for u, to in enumerate(lists) for d, _ in to], dtype=np.int32).reshape(-1, 2)
    wgt = np.array([w for to in lists for _, w in to], dtype=F)
    return idx, wgt


def triangle_unrounded_scatter(f, wrap_u, wrap_v):
    """The accumulation as the reference runs it (:1229-1256): source rows, source columns, the row's destinations, the column's."""
    h, w = f.shape[:2]
    nw, nh = max(1, w >> 1), max(1, h >> 1)
    xl, yl = triangle_lists(w, nw, wrap_u), triangle_lists(h, nh, wrap_v)
    acc = np.zeros((nh, nw, 4), dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        for y in range(h):
            for x in range(w):
                for v, yw in yl[y]:
                    for u, xw in xl[x]:
                        wgt = yw * xw
                        t = f[y, x] * wgt
                        acc[v, u] = t + acc[v, u]
    return acc


def _by_rank(lists, dest):
    """For every destination the sources that reach it in order of arrival: (rank, dest) int64 sources and fp32 weights, a bool mask."""
    per = [[] for _ in range(dest)]
    for u, to in enumerate(lists):
        seen = set()
        for d, w in to:
            if d in seen:
                return None                                          # one source, one destination, two entries: the scalar path
            seen.add(d)
            per[d].append((u, w))
    ranks = max(len(p) for p in per)
    src = np.zeros((ranks, dest), dtype=np.int64)
    wgt = np.zeros((ranks, dest), dtype=F)
    have = np.zeros((ranks, dest), dtype=bool)
    for d, p in enumerate(per):
        for r, (u, w) in enumerate(p):
            src[r, d], wgt[r, d], have[r, d] = u, w, True
    return src, wgt, have


def triangle_unrounded(f, wrap_u, wrap_v):
    h, w = f.shape[:2]
    nw, nh = max(1, w >> 1), max(1, h >> 1)
    xl, yl = triangle_lists(w, nw, wrap_u), triangle_lists(h, nh, wrap_v)
    ranked = _by_rank(xl, nw)
    if ranked is None or any(len({v for v, _ in to}) != len(to) for to in yl):
        return triangle_unrounded_scatter(f, wrap_u, wrap_v)
    src, wgt, have = ranked
    acc = np.zeros((nh, nw, 4), dtype=F)
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


def store_rgba8_signed(v):
    """(uint8_t)min(max(v, 0.0f) + 0.5f, 255.0f): tests/_mipgen.py's store for every v >= 0."""
    t = np.maximum(v, F(0.0))
    t = t + F(0.5)
    t = np.minimum(t, F(255.0))
    return t.astype(np.uint8)


def widen(img, kind):
    if kind == "srgb":
        return S.widen(img)
    assert img.dtype == (np.uint16 if kind == "rgba16f" else np.uint8)
    return M.widen(img)


def store(v, kind):
    if kind == "rgba16f":
        return M.store_rgba16f(v)
    if kind == "rgba8":
        return store_rgba8_signed(v)
    out = np.empty(v.shape, dtype=np.uint8)
    out[..., :3] = S.encode(v[..., :3])
    out[..., 3] = store_rgba8_signed(v[..., 3])
    return out


def level(src, filt, wrap="", kind=None):
    kind = kind or ("rgba16f" if src.dtype == np.uint16 else "rgba8")
    step = cubic_unrounded if filt == "cubic" else triangle_unrounded
    return np.ascontiguousarray(store(step(widen(src, kind), "u" in wrap, "v" in wrap), kind))


def chain(base, filt, wrap="", kind=None, levels=0):
    """[base, level 1, ...]: `filt` ("cubic" or "triangle") on every level, level l from level l-1 as stored."""
    h, w = base.shape[:2]
    out = [np.ascontiguousarray(base)]
    for _ in range(1, levels or M.levels_of(w, h)):
        out.append(level(out[-1], filt, wrap, kind))
    return out


def seeded_half_image(h, w, seed):
    """Finite RGBA16F content for the recording and the tests: tests/_mipgen.py's both-signs noise, plus denormals and magnitudes near
    65504 next to small ones, so that cubic overshoot meets the store's clamp."""
    bits = M.seeded_half_image(h, w, seed)
    rng = np.random.default_rng(seed + 1000)
    pick = rng.random((h, w, 4))
    sign = (rng.integers(0, 2, (h, w, 4)) << 15).astype(np.uint16)
    bits = np.where(pick < 0.06, (rng.integers(1, 0x400, (h, w, 4)).astype(np.uint16) | sign), bits)            # denormals
    bits = np.where(pick > 0.94, (rng.integers(0x7B00, 0x7C00, (h, w, 4)).astype(np.uint16) | sign), bits)      # 57344 .. 65504
    return np.ascontiguousarray(bits.astype(np.uint16))


def seeded_byte_image(h, w, seed):
    """RGBA8 content with flat runs at 0 and 255 beside noise: cubic overshoot on both ends of the code range."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    pick = rng.random((h, w, 1))
    img = np.where(pick < 0.2, np.uint8(0), np.where(pick > 0.8, np.uint8(255), img))
    return np.ascontiguousarray(img.astype(np.uint8))
