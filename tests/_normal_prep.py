"""The checker of the normal-map stages (include/itw_dispatch.h: ITW_NORMAL_*): a plain numpy restatement of the per-texel definition,
IntelPlugin.cpp:1506-1545 (FlipXYChannelNormalMap) and :1550-1613 (NormalizeNormalMapChain).  float32 arrays, one operation per line, so
every operation is rounded on its own; astype(np.uint8) / astype(np.float16) at the end (numpy's float32 -> float16 rounds to nearest
even).  Not a test module: tests import it."""
import numpy as np

FLIP_X, FLIP_Y, NORMALIZE = 1, 2, 4


def prepare_rgba8(img, ops):
    """img: uint8 array (..., 4).  Returns the prepared copy."""
    out = np.array(img, dtype=np.uint8, copy=True)
    if ops & FLIP_X:
        out[..., 0] = 255 - out[..., 0]
    if ops & FLIP_Y:
        out[..., 1] = 255 - out[..., 1]
    if ops & NORMALIZE:
        r = (out[..., 0].astype(np.int32) - 128).astype(np.float32)
        g = (out[..., 1].astype(np.int32) - 128).astype(np.float32)
        b = (out[..., 2].astype(np.int32) - 128).astype(np.float32)
        rr = r * r
        gg = g * g
        bb = b * b
        s2 = rr + gg
        s3 = s2 + bb
        m = np.sqrt(s3)
        ok = m > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.float32(127.0) / m
            nr = r * s
            ng = g * s
            nb = b * s
            nr = nr + np.float32(128.0)
            ng = ng + np.float32(128.0)
            nb = nb + np.float32(128.0)
        assert rr.dtype == s.dtype == nb.dtype == np.float32
        out[..., 0] = np.where(ok, nr, np.float32(128.0)).astype(np.uint8)
        out[..., 1] = np.where(ok, ng, np.float32(128.0)).astype(np.uint8)
        out[..., 2] = np.where(ok, nb, np.float32(255.0)).astype(np.uint8)
    return out


def prepare_rgba16f(img, ops):
    """img: uint16 array (..., 4) of half bit patterns.  Returns the prepared copy (bit patterns)."""
    out = np.array(img, dtype=np.uint16, copy=True)
    h = out.view(np.float16)
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        if ops & FLIP_X:
            v = h[..., 0].astype(np.float32)
            v = one - v
            h[..., 0] = v.astype(np.float16)
        if ops & FLIP_Y:
            v = h[..., 1].astype(np.float32)
            v = one - v
            h[..., 1] = v.astype(np.float16)
        if ops & NORMALIZE:
            r = h[..., 0].astype(np.float32)
            g = h[..., 1].astype(np.float32)
            b = h[..., 2].astype(np.float32)
            rr = r * r
            gg = g * g
            bb = b * b
            s2 = rr + gg
            s3 = s2 + bb
            m = np.sqrt(s3)
            ok = m > 0                                   # false for a NaN length, as in the reference
            s = one / m
            nr = r * s
            ng = g * s
            nb = b * s
            assert s.dtype == nb.dtype == np.float32
            zero = np.zeros((), np.uint16)
            out[..., 0] = np.where(ok, nr.astype(np.float16).view(np.uint16), zero)
            out[..., 1] = np.where(ok, ng.astype(np.float16).view(np.uint16), zero)
            out[..., 2] = np.where(ok, nb.astype(np.float16).view(np.uint16), np.uint16(0x3C00))
    return out


def prepare(img, ops):
    return prepare_rgba16f(img, ops) if img.dtype.itemsize == 2 else prepare_rgba8(img, ops)


def all_triples():
    """The 4096 x 4096 RGBA8 surface that holds every RGB triple once, R outermost and B innermost in raster order, alpha a varying pattern."""
    i = np.arange(1 << 24, dtype=np.uint32)
    img = np.empty((1 << 24, 4), np.uint8)
    img[:, 0] = i >> 16
    img[:, 1] = (i >> 8) & 255
    img[:, 2] = i & 255
    img[:, 3] = (i * np.uint32(2654435761) >> np.uint32(24)).astype(np.uint8)
    return img.reshape(4096, 4096, 4)
