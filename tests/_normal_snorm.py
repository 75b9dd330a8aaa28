"""The checker of the signed normal-map path (include/itw_dispatch.h, "signed normal sources"): a plain numpy restatement of the per-texel
definition.  float32 arrays, one operation per line, so every operation is rounded on its own; np.rint rounds to nearest even; NaN -> 0 is
explicit.  Not a test module: tests import it."""
import numpy as np

FLIP_X, FLIP_Y, NORMALIZE = 1, 2, 4
f32 = np.float32


def texel_bytes(img):
    """int8 -> 4 (RGBA8_SNORM), 2-byte elements -> 8 (RGBA16F), float32 -> 16 (RGBA32F)."""
    return {1: 4, 2: 8, 4: 16}[np.asarray(img).dtype.itemsize]


def load(img):
    """(..., 4) int8 codes, float16 / uint16 half bits, or float32 -> the float32 working values."""
    img = np.asarray(img)
    if img.dtype == np.int8:
        v = img.astype(f32)
        v = v * (f32(1.0) / f32(127.0))
        return np.maximum(v, f32(-1.0))
    if img.dtype.itemsize == 2:
        return img.view(np.float16).astype(f32)
    assert img.dtype == np.float32
    return np.array(img, copy=True)


def apply_ops(v, ops):
    """The flips, then the normalise, on float32 working values (..., 4); returns a new array."""
    v = np.array(v, dtype=f32, copy=True)
    if ops & FLIP_X:
        v[..., 0] = -v[..., 0]
    if ops & FLIP_Y:
        v[..., 1] = -v[..., 1]
    if ops & NORMALIZE:
        x = v[..., 0].copy()
        y = v[..., 1].copy()
        z = v[..., 2].copy()
        with np.errstate(all="ignore"):
            xx = x * x
            yy = y * y
            zz = z * z
            s2 = xx + yy
            s3 = s2 + zz
            m = np.sqrt(s3)
            ok = m > 0                                   # false for a NaN length
            s = f32(1.0) / m
            nx = x * s
            ny = y * s
            nz = z * s
        assert xx.dtype == s3.dtype == m.dtype == s.dtype == nz.dtype == np.float32
        v[..., 0] = np.where(ok, nx, f32(0.0))
        v[..., 1] = np.where(ok, ny, f32(0.0))
        v[..., 2] = np.where(ok, nz, f32(1.0))
    return v


def quantize_values(v):
    """float32 working values -> int8 codes: NaN -> 0, clamp to [-1, 1], * 127, round to nearest even."""
    v = np.asarray(v, dtype=f32)
    nan = np.isnan(v)
    c = np.where(nan, f32(0.0), v)
    c = np.maximum(c, f32(-1.0))
    c = np.minimum(c, f32(1.0))
    p = c * f32(127.0)
    assert p.dtype == np.float32
    r = np.rint(p)
    return r.astype(np.int32).astype(np.int8)


def quantize(img, ops=0):
    """The RGBA8_SNORM image (int8, same shape) the definition makes of a signed normal source."""
    return quantize_values(apply_ops(load(img), ops))


# ---- seeded content the GPU tests share ----------------------------------------------------------------------------------------------------
KINDS = ("int8", "half", "float")
_content = {}


def content(kind, h, w, seed):
    """(h, w, 4) of the kind: unit-ish vectors with noise, and a share of zero vectors, exact +-1, out-of-range values, NaN (half / float) or
    -128 (int8)"""
    key = (kind, h, w, seed)
    if key not in _content:
        rng = np.random.default_rng(seed)
        v = rng.normal(0, 0.45, (h, w, 4)).astype(f32)
        v[..., 2] = np.abs(v[..., 2]) + f32(0.3)
        k = rng.integers(0, 24, (h, w))
        v[k == 0, :3] = 0
        v[k == 1, :2] = [1, -1]
        v[k == 2, :3] = [-1.5, 2.5, 0]
        v[k == 3] = v[k == 3] * f32(0.01)
        if kind == "int8":
            a = np.clip(np.rint(v * 127), -128, 127).astype(np.int8)
            a[k == 4, :2] = [-128, 127]
        elif kind == "half":
            v[k == 4, 0] = np.nan
            a = v.astype(np.float16).view(np.uint16)
        else:
            v[k == 4, 1] = np.nan
            v[k == 5, 0] = np.inf
            a = v
        _content[key] = np.ascontiguousarray(a)
    return _content[key]


def torch_of(a, gpu):
    """numpy array -> CUDA tensor of the same bytes (uint16 half bits travel as int16)"""
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(gpu)
