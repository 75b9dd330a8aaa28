"""The reference's BC2 codec for the tests: D3DXEncodeBC2 / D3DXDecodeBC2 of oracle/_ref/libdxtex_bc_ref.so (BC.cpp compiled unmodified by
oracle/ref_build/Makefile), bound by their C++ names as tests/_dxtex_bc1.py binds the BC1 pair; a numpy model of the encoder's alpha half
(BC.cpp:834-878: fp32, one rounding per operation, vectorised over blocks) that also says, per block, what the dither did -- the colour half
is _dxtex_bc1.model with alpha_ref 0 and without DITHER_A, which is what D3DXEncodeBC2 calls; the content the CPU and GPU tests share; the
blocks the decode tests decode; and the recorded streams of tests/golden/bc2_ref.npz (tools/gen_golden_bc2.py).

Texel conversion (include/itw_dispatch.h): an RGBA8 code v is the float (float)v * (1.0f / 255.0f).  Partial blocks are filled as
DirectXTexCompress.cpp:140-168 fills them (_dxtex_snorm.block_texels)."""
import ctypes as C
import os
import subprocess

import numpy as np

import _dxtex_bc1 as B
from _dxtex_bc1 import DITHER_A, DITHER_RGB, FLAG_SETS, UNIFORM, F, _diffuse, _trunc, to_float      # noqa: F401
from _dxtex_snorm import ROOT, _aligned, block_texels

GOLDEN = os.path.join(ROOT, "tests", "golden", "bc2_ref.npz")
_ENC = "_ZN7DirectX13D3DXEncodeBC2EPhPKNS_8XMVECTOREm"
_DEC = "_ZN7DirectX13D3DXDecodeBC2EPNS_8XMVECTOREPKh"
_bound = False


def lib():
    """The bound library; skips the calling test where it is absent and cannot be built (the golden streams are compared either way)."""
    global _bound
    L = B.lib()
    if not _bound:
        e = getattr(L, _ENC)
        e.argtypes = [C.c_void_p, C.c_void_p, C.c_ulong]
        e.restype = None
        d = getattr(L, _DEC)
        d.argtypes = [C.c_void_p, C.c_void_p]
        d.restype = None
        _bound = True
    return L


def encode_blocks(texels, flags):
    """texels (n, 16, 4) uint8 -> (n, 16) uint8 through the reference's D3DXEncodeBC2."""
    fn = getattr(lib(), _ENC)
    texels = np.asarray(texels)
    assert texels.dtype == np.uint8 and texels.shape[1:] == (16, 4)
    n = texels.shape[0]
    px = _aligned((n, 16, 4), np.float32)
    px[...] = to_float(texels)
    out = np.zeros((n, 16), dtype=np.uint8)
    p, o = px.ctypes.data, out.ctypes.data
    for i in range(n):
        fn(o + i * 16, p + i * 256, int(flags))
    return out


def encode(img, flags=0):
    """The stream DirectX::Compress gives an RGBA8 image of any size: (H, W, 4) uint8 -> uint8 blocks, flat."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    return encode_blocks(block_texels(img), flags).reshape(-1)


def decode(blocks):
    """blocks -> (n, 16, 4) float32, the reference's D3DXDecodeBC2."""
    fn = getattr(lib(), _DEC)
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, 16)
    n = blocks.shape[0]
    out = _aligned((n, 16, 4), np.float32)
    p, o = blocks.ctypes.data, out.ctypes.data
    for i in range(n):
        fn(o + i * 256, p + i * 16)
    return np.array(out)


# ---- content ------------------------------------------------------------------------------------------------------------------------

def alpha_blocks():
    """(8, 128, 4) uint8, 64 constructed blocks for what the alpha half can do: blocks 0..15 hold the 256 alpha codes (block b, texel i:
    16 b + i); 16..31 an opaque texel behind texels whose differences are positive (alpha 8 rounds down to nibble 0 and leaves + 8/255),
    so that under DITHER_A fAlph rises above 1; 32..47 a zero texel behind negative differences (alpha 9 rounds up to nibble 1 and leaves
    - 8/255), so that fAlph falls below 0; 48..63 random alpha.  Colour: noise (the colour half has its own content)."""
    rng = np.random.default_rng(2050)
    blocks = np.zeros((64, 16, 4), dtype=np.uint8)
    blocks[..., :3] = rng.integers(0, 256, (64, 16, 3))
    for b in range(16):
        blocks[b, :, 3] = 16 * b + np.arange(16)
    for b in range(16, 32):
        a = 8 + 17 * rng.integers(0, 15, 16)                    # 17 k + 8: the largest positive difference a lone texel leaves
        a[rng.integers(1, 16, 1 + b % 4)] = 255
        a[5] = 255                                                 # behind texels 0, 1, 2, 4
        blocks[b, :, 3] = a
    for b in range(32, 48):
        a = 9 + 17 * rng.integers(0, 15, 16)                    # 17 k + 9: the largest negative one
        a[rng.integers(1, 16, 1 + b % 4)] = 0
        a[5] = 0
        blocks[b, :, 3] = a
    blocks[48:, :, 3] = rng.integers(0, 256, (16, 16))
    return np.ascontiguousarray(blocks.reshape(2, 32, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(8, 128, 4))


_content = None


def content():
    """name -> image: what the CPU model test, the golden file and the GPU tests all encode: _dxtex_bc1's shared content plus alpha_blocks()."""
    global _content
    if _content is None:
        _content = dict(B.content())
        _content["alpha"] = alpha_blocks()
    return _content


def decode_test_blocks():
    """(64, 16) uint8: BC2 blocks for the decoders.  Block k < 48: the alpha nibble of texel i is (i + k) & 15 -- every value in every
    position over k = 0..15 --, its colour index (i + k) & 3 -- all four in every block --, and its endpoints c0 > c1 (k % 3 == 0), c0 < c1
    (k % 3 == 1: a BC1 decoder would show index 3 black and transparent; BC2 has no 3-colour mode) or c0 == c1 (k % 3 == 2).  48..63: random bits."""
    rng = np.random.default_rng(74)
    out = np.zeros((64, 4), dtype=np.uint32)
    for k in range(48):
        nib = (np.arange(16) + k) & 15
        out[k, 0] = sum(int(nib[i]) << (4 * i) for i in range(8))
        out[k, 1] = sum(int(nib[8 + i]) << (4 * i) for i in range(8))
        lo, hi = sorted(int(v) for v in rng.choice(65536, 2, replace=False))
        c0, c1 = ((hi, lo), (lo, hi), (hi, hi))[k % 3]
        out[k, 2] = c0 | (c1 << 16)
        out[k, 3] = sum(((i + k) & 3) << (2 * i) for i in range(16))
    out[48:] = rng.integers(0, 1 << 32, (16, 4), dtype=np.uint64).astype(np.uint32)
    return np.ascontiguousarray(out.astype("<u4")).view(np.uint8).reshape(64, 16)


SIZES = ((1, 1), (3, 5), (5, 3), (4, 4), (61, 75))      # (h, w): the partial-block cases, recorded as "size.<h>x<w>.<flags>" for SIZE_FLAGS
SIZE_FLAGS = (0, DITHER_RGB | DITHER_A)


def cutout(h, w, seed=7):
    """Cut-out content of any size: colour ramps with noise under an alpha plane of discs with soft rims (every alpha code between the
    transparent and the opaque areas occurs)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.zeros((h, w, 4), dtype=np.uint8)
    img[..., 0] = (x * 255 / max(1, w - 1)).astype(np.uint8)
    img[..., 1] = (y * 255 / max(1, h - 1)).astype(np.uint8)
    img[..., 2] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    a = np.zeros((h, w), dtype=np.float32)
    for _ in range(6):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(4, max(5, min(h, w) / 3))
        a = np.maximum(a, np.clip((r - np.hypot(y - cy, x - cx)) / 3.0 + 0.5, 0, 1))
    img[..., 3] = np.rint(a * 255).astype(np.uint8)
    return img


def size_image(h, w):
    return cutout(h, w, seed=h * 100 + w)


def size_key(h, w, flags):
    return "size.%dx%d.%05x" % (h, w, flags)


def golden_key(name, flags):
    return "%s.%05x" % (name, flags)


_golden = None


def golden():
    """The reference's recordings (tools/gen_golden_bc2.py): golden_key(...) -> uint8 stream; "decode.blocks" / "decode.ref": decode_test_blocks()
    and D3DXDecodeBC2 of them, (64, 16, 4) float32.  A missing file fails the caller."""
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


# ---- the model: D3DXEncodeBC2 (BC.cpp:820-890) in numpy -----------------------------------------------------------------------------------

ALPHA_PATHS = ("raised", "lowered", "above_one", "below_zero", "spill")


def alpha_model(texels, flags):
    """texels (n, 16, 4) uint8 -> ((n, 8) uint8: bitmap[0], bitmap[1], {what: (n,) bool}).  Per block, under DITHER_A: `raised` / `lowered`: a
    nibble is above / below the one the texel has without the flag; `above_one` / `below_zero`: a texel's fAlph, its alpha plus the
    diffused error, left 0..1; `spill`: a u above 15 (the source's `u << 28` would then reach the texels before it; the words are built in
    32 bits as the source builds them, so the model spills as it does)."""
    texels = np.asarray(texels)
    n = texels.shape[0]
    a = to_float(texels)[..., 3]
    da = bool(flags & DITHER_A)
    bm = np.zeros((n, 2), dtype=np.uint32)
    E = np.zeros((n, 16), dtype=F)
    paths = {k: np.zeros(n, dtype=bool) for k in ALPHA_PATHS}
    with np.errstate(all="ignore"):
        for i in range(16):
            alph = a[:, i] + E[:, i] if da else a[:, i]
            u = _trunc(alph * F(15.0) + F(0.5)).astype(np.uint32)
            plain = _trunc(a[:, i] * F(15.0) + F(0.5)).astype(np.uint32)
            bm[:, i >> 3] = (bm[:, i >> 3] >> np.uint32(4)) | (u << np.uint32(28))
            paths["raised"] |= u.astype(np.int64) > plain
            paths["lowered"] |= u.astype(np.int64) < plain
            paths["above_one"] |= alph > F(1.0)
            paths["below_zero"] |= alph < F(0.0)
            paths["spill"] |= u > 15
            if da:
                _diffuse(E, i, alph - u.astype(F) * (F(1.0) / F(15.0)))
    return np.ascontiguousarray(bm.astype("<u4")).view(np.uint8).reshape(n, 8), paths


def model(texels, flags):
    """texels (n, 16, 4) uint8 -> ((n, 16) uint8 blocks, paths of the alpha half, paths of the colour half)."""
    alpha, apaths = alpha_model(texels, flags)
    colour, cpaths = B.model(texels, 0.0, flags & ~DITHER_A)          # EncodeBC1(..., false, 0.f, flags), which never reads DITHER_A
    return np.concatenate([alpha, colour], axis=1), apaths, cpaths


# ---- the kernel's text on the host (tools/bc2_host_check.cpp over csrc/bc2_core.hpp) -----------------------------------------------------

def build_host_check(tmp_dir, extra=()):
    exe = os.path.join(str(tmp_dir), "bc2_host_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", *extra, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "bc2_host_check.cpp"), "-o", exe], check=True)
    return exe


def host_check_encode(exe, tmp_dir, texels, flags):
    src, dst = os.path.join(str(tmp_dir), "texels.bin"), os.path.join(str(tmp_dir), "blocks.bin")
    np.ascontiguousarray(texels, dtype=np.uint8).tofile(src)
    subprocess.run([exe, src, dst, str(flags)], check=True)
    return np.fromfile(dst, dtype=np.uint8).reshape(-1, 16)


# ---- a BC2 decoder from the format's definition, in numpy (what the device decoder must give, code for code) -----------------------------

def np_decode(blocks, h, w):
    """blocks: the stream of a h x w image (ceil(w/4) x ceil(h/4) blocks) -> (h, w, 4) uint8.  Colour: always the four-colour palette --
    5:6:5 expanded by bit replication, the two inner colours (2 a + b + 1) // 3 --, whatever the order of the endpoints; alpha: nibble * 17."""
    by, bx = (h + 3) // 4, (w + 3) // 4
    wd = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1)[:by * bx * 16].view("<u4").reshape(-1, 4).astype(np.int64)
    n = wd.shape[0]
    pal = np.zeros((n, 4, 3), dtype=np.int64)
    for k, c in enumerate((wd[:, 2] & 0xFFFF, wd[:, 2] >> 16)):
        r, g, b = (c >> 11) & 31, (c >> 5) & 63, c & 31
        pal[:, k] = np.stack([(r << 3) | (r >> 2), (g << 2) | (g >> 4), (b << 3) | (b >> 2)], axis=1)
    pal[:, 2] = (2 * pal[:, 0] + pal[:, 1] + 1) // 3
    pal[:, 3] = (pal[:, 0] + 2 * pal[:, 1] + 1) // 3
    out = np.zeros((n, 16, 4), dtype=np.uint8)
    rows = np.arange(n)
    for i in range(16):
        out[:, i, :3] = pal[rows, (wd[:, 3] >> (2 * i)) & 3]
        out[:, i, 3] = ((wd[:, i >> 3] >> (4 * (i & 7))) & 15) * 17
    img = out.reshape(by, bx, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(by * 4, bx * 4, 4)
    return np.ascontiguousarray(img[:h, :w])
