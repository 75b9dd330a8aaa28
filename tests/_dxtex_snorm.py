"""The reference's own BC4_SNORM / BC5_SNORM codecs for the tests: D3DXEncodeBC4S/BC5S and D3DXDecodeBC4S/BC5S of
oracle/_ref/libdxtex_bc_ref.so (BC.cpp, BC4BC5.cpp, BC6HBC7.cpp compiled unmodified by oracle/ref_build/Makefile), bound by their C++
names.  XMVECTOR is four floats there, so a (16, 4) float32 array is a block's sixteen texels.

Texel conversion (include/itw_bc45.h): an int8 code v is the float max((float)v * (1.0f / 127.0f), -1.0f), DirectXMath's SSE XMLoadByteN4.
Partial blocks are filled as DirectXTexCompress.cpp:140-168 fills them, in its order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "oracle", "_ref", "libdxtex_bc_ref.so")
BPB = {1: 8, 2: 16}
_NAMES = {("enc", 1): "_ZN7DirectX14D3DXEncodeBC4SEPhPKNS_8XMVECTOREm", ("enc", 2): "_ZN7DirectX14D3DXEncodeBC5SEPhPKNS_8XMVECTOREm",
          ("dec", 1): "_ZN7DirectX14D3DXDecodeBC4SEPNS_8XMVECTOREPKh", ("dec", 2): "_ZN7DirectX14D3DXDecodeBC5SEPNS_8XMVECTOREPKh"}
_lib = None


def lib():
    """The bound library; skips the calling test where it is absent and cannot be built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            if not os.path.exists("/root/reference/3rdParty/DirectXTex/DirectXTex/BC4BC5.cpp"):
                pytest.skip("oracle/_ref/libdxtex_bc_ref.so not prebuilt and /root/reference absent")
            subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True)
            subprocess.run(["make", "-C", os.path.join(ROOT, "oracle", "ref_build")], check=True)
        L = C.CDLL(LIB)
        for nch in (1, 2):
            e = getattr(L, _NAMES[("enc", nch)])
            e.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
            e.restype = None
            d = getattr(L, _NAMES[("dec", nch)])
            d.argtypes = [C.c_void_p, C.c_void_p]
            d.restype = None
        _lib = L
    return _lib


def _aligned(shape, dtype, align=64):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.zeros(n + align, dtype=np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + n].view(dtype).reshape(shape)


def to_float(codes):
    """int8 codes -> the floats the encoder sees, in fp32."""
    return np.maximum(np.asarray(codes, dtype=np.int8).astype(np.float32) * (np.float32(1.0) / np.float32(127.0)), np.float32(-1.0))


def _fill(valid):
    """Source column / row of each of a block's four, when only the first `valid` exist (uSrc = {0, 0, 0, 1}, applied in order)."""
    src = list(range(valid))
    for s in range(valid, 4):
        src.append(src[(0, 0, 0, 1)[s]])
    return src


def block_texels(img):
    """(H, W, C) -> (blocks, 16, C) in raster block order with DirectXTex's partial-block fill, any H, W >= 1."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    by, bx = (h + 3) // 4, (w + 3) // 4
    rows = np.concatenate([4 * y + np.array(_fill(min(4, h - 4 * y))) for y in range(by)])
    cols = np.concatenate([4 * x + np.array(_fill(min(4, w - 4 * x))) for x in range(bx)])
    full = img[rows][:, cols]
    return full.reshape(by, 4, bx, 4, -1).transpose(0, 2, 1, 3, 4).reshape(by * bx, 16, -1)


def encode_blocks(nch, texels):
    """texels: (n, 16, >= nch) int8 -> (n, 8 * nch) uint8 through D3DXEncodeBC4S / BC5S."""
    L = lib()
    fn = getattr(L, _NAMES[("enc", nch)])
    texels = np.asarray(texels)
    assert texels.dtype == np.int8
    n = texels.shape[0]
    px = _aligned((n, 16, 4), np.float32)
    px[..., :nch] = to_float(texels[..., :nch])
    px[..., 3] = 1.0
    out = np.zeros((n, BPB[nch]), dtype=np.uint8)
    p, o = px.ctypes.data, out.ctypes.data
    for i in range(n):
        fn(o + i * BPB[nch], p + i * 256, 0)
    return out


def encode(nch, img):
    """The stream DirectX::Compress gives an RGBA8_SNORM image: img (H, W, 4) int8 -> uint8 blocks, flat."""
    img = np.asarray(img)
    assert img.dtype == np.int8 and img.ndim == 3
    return encode_blocks(nch, block_texels(img)).reshape(-1)


def decode(nch, blocks):
    """blocks -> (n, 16, 4) float32, D3DXDecodeBC4S / BC5S."""
    L = lib()
    fn = getattr(L, _NAMES[("dec", nch)])
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, BPB[nch])
    n = blocks.shape[0]
    out = _aligned((n, 16, 4), np.float32)
    p, o = blocks.ctypes.data, out.ctypes.data
    for i in range(n):
        fn(o + i * 256, p + i * BPB[nch])
    return np.array(out)


_levels = None


def levels():
    """(256, 256, 8) float32: the eight decoded levels of every endpoint pair [r0 byte, r1 byte], from the reference's decoder: a block
    whose first eight indices are 0..7."""
    global _levels
    if _levels is None:
        idx = sum(k << (3 * k) for k in range(8))
        blocks = np.zeros((65536, 8), dtype=np.uint8)
        pair = np.arange(65536)
        blocks[:, 0] = pair >> 8
        blocks[:, 1] = pair & 255
        blocks[:, 2:8] = np.frombuffer(int(idx).to_bytes(6, "little"), dtype=np.uint8)
        _levels = np.ascontiguousarray(decode(1, blocks)[:, :8, 0]).reshape(256, 256, 8)
    return _levels


# ---- seeded content ---------------------------------------------------------------------------------------------------------------

def _boundary_heavy(h, w, seed):
    """tests/test_gpu_parity_bc4_bc5.py's generator, restated (shared by the GPU tests and tools/gen_golden_bc45_snorm.py): many exact
    0 / 255 texels, flat blocks, blocks whose interior values collapse (fX == fY), two-level blocks.  XOR 0x80 turns its codes into signed ones of the same structure (0 -> -128, 255 -> 127)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    kind = rng.integers(0, 6, (h // 4, w // 4))
    k = np.repeat(np.repeat(kind, 4, axis=0), 4, axis=1)[..., None]
    base = np.repeat(np.repeat(rng.integers(0, 256, (h // 4, w // 4, 4), dtype=np.uint8), 4, axis=0), 4, axis=1)
    img = np.where(k == 1, base, img)
    img = np.where(k == 2, np.where(img < 90, 0, np.where(img > 170, 255, base)), img)
    img = np.where(k == 3, np.where(img < 128, 0, 255), img)
    img = np.where(k == 4, np.clip(base.astype(np.int32) + (img.astype(np.int32) % 7) - 3, 0, 255).astype(np.uint8), img)
    img = np.where(k == 5, np.where(img < 40, 0, img), img)
    return np.ascontiguousarray(img.astype(np.uint8))


def boundary_heavy_snorm():
    """(128, 128, 4) int8: the boundary-heavy content in signed codes."""
    return np.ascontiguousarray((_boundary_heavy(128, 128, 45) ^ 0x80).view(np.int8))


# ---- the model the tests share: numpy restatements, pinned to the functions above by tests/test_bc45_snorm_reference.py ----------

def model_levels():
    """BC4_SNORM::DecodeFromIndex (BC4BC5.cpp:106-131) in fp32, one rounding per operation: (256, 256, 8) float32 by endpoint bytes."""
    f32 = np.float32
    raw = np.arange(256).astype(np.uint8).view(np.int8).astype(np.int32)
    s = np.where(raw == -128, -127, raw).astype(f32) / f32(127.0)
    f0, f1 = s[:, None], s[None, :]
    eight = raw[:, None] > raw[None, :]
    g = np.empty((256, 256, 8), dtype=f32)
    g[..., 0] = f0
    g[..., 1] = f1
    for k in range(1, 7):
        v8 = (f0 * f32(7 - k) + f1 * f32(k)) / f32(7.0)
        v6 = (f0 * f32(5 - k) + f1 * f32(k)) / f32(5.0) if k <= 4 else np.full((256, 256), -1.0 if k == 5 else 1.0, dtype=f32)
        g[..., k + 1] = np.where(eight, v8, v6)
    return g


def integer_levels():
    """The decoders' 8-bit rule (include/itw_decode.h): (256, 256, 8) int32 by endpoint bytes."""
    raw = np.arange(256).astype(np.uint8).view(np.int8).astype(np.int64)
    s = np.where(raw == -128, -127, raw)
    s0, s1 = s[:, None], s[None, :]
    eight = raw[:, None] > raw[None, :]
    a = np.empty((256, 256, 8), dtype=np.int64)
    a[..., 0] = s0
    a[..., 1] = s1
    for i in range(1, 7):
        v8 = (2 * ((7 - i) * s0 + i * s1) + 7) // 14              # floor((2n + d) / (2d)): numpy's // floors
        v6 = (2 * ((5 - i) * s0 + i * s1) + 5) // 10 if i <= 4 else np.full((256, 256), -127 if i == 5 else 127)
        a[..., 1 + i] = np.where(eight, v8, v6)
    return a.astype(np.int32)


def closest_table(g):
    """F[r0 byte, r1 byte, code byte] uint8: the first index with the strictly smallest |level - t| (FindClosestSNORM) over levels g."""
    t = to_float(np.arange(256).astype(np.uint8).view(np.int8))                 # by code byte
    F = np.empty((256, 256, 256), dtype=np.uint8)
    for r0 in range(256):
        d = np.abs(g[r0][:, None, :] - t[None, :, None])                        # (r1, code, 8)
        F[r0] = np.argmin(d, axis=2)                                            # argmin: the first minimum
    return F


def run_counts(F):
    """(256, 256): number of runs of F[r0, r1, :] with the codes in signed order (-128 .. 127)."""
    order = np.arange(-128, 128).astype(np.int8).view(np.uint8)
    G = F[:, :, order]
    return 1 + (G[:, :, 1:] != G[:, :, :-1]).sum(axis=2)


def decode_int8(nch, blocks, width, height):
    """The integer rule applied to a stream: (H, W, 4) int8 (R, G or 0, 0, 127), cropped to width x height."""
    lv = integer_levels()
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, BPB[nch])
    by, bx = (height + 3) // 4, (width + 3) // 4
    assert blocks.shape[0] == by * bx
    out = np.zeros((blocks.shape[0], 16, 4), dtype=np.int8)
    out[..., 3] = 127
    for c in range(nch):
        b = blocks[:, 8 * c:8 * c + 8]
        bits = np.zeros(blocks.shape[0], dtype=np.uint64)
        for k in range(6):
            bits |= b[:, 2 + k].astype(np.uint64) << np.uint64(8 * k)
        idx = np.stack([(bits >> np.uint64(3 * k)) & np.uint64(7) for k in range(16)], axis=1).astype(np.int64)
        out[..., c] = lv[b[:, 0].astype(np.int64)[:, None], b[:, 1].astype(np.int64)[:, None], idx].astype(np.int8)
    img = out.reshape(by, bx, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(by * 4, bx * 4, 4)
    return np.ascontiguousarray(img[:height, :width])
