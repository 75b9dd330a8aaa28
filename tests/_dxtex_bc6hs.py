"""The signed reading of BC6H for the tests: D3DXDecodeBC6HS of oracle/_ref/libdxtex_bc_ref.so (BC6HBC7.cpp compiled unmodified by
oracle/ref_build/Makefile), bound by its C++ name as tests/_dxtex_bc2.py binds the BC2 pair; a numpy decoder written from the six steps of
include/itw_decode.h (sign extension, TransformInverse, Unquantize, interpolation, FinishUnquantize, INT2F16) over the committed bit layout
oracle/bc6h_layout.h and the partition tables of oracle/bc7_tables.h, which also says per block what happened in it; the block sets the CPU
and GPU tests share; and the recording tests/golden/bc6hs_ref.npz (tools/gen_golden_bc6hs.py).  Nothing here reads the reference tree.

Texels are uint16 half bit patterns, (n, 16, 4), alpha 0x3C00."""
import ctypes as C
import os
import re

import numpy as np

import _block_sweep as S
import _dxtex_bc1 as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bc6hs_ref.npz")
FORMAT = 0x8E8E                                                  # ITW_FORMAT_BC6H_SIGNED
_DEC = "_ZN7DirectX15D3DXDecodeBC6HSEPNS_8XMVECTOREPKh"
_ENC = "_ZN7DirectX15D3DXEncodeBC6HSEPhPKNS_8XMVECTOREm"
W3 = np.array([0, 9, 18, 27, 37, 46, 55, 64], dtype=np.int64)
W4 = np.array([0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64], dtype=np.int64)
SEED = 20261021


# ---- the committed tables ----------------------------------------------------------------------------------------------------------------

def _layouts():
    """[(prefix, two_regions, transformed, base_bits[3], delta_bits[3], slot[82])] for modes 0..13, from oracle/bc6h_layout.h."""
    text = open(os.path.join(ROOT, "oracle", "bc6h_layout.h")).read()
    rows = re.findall(r"\{\s*(0x[0-9a-fA-F]+),\s*(\d+),\s*(\d+),\s*\{(\d+),(\d+),(\d+)\},\s*\{(\d+),(\d+),(\d+)\},\s*\{([^}]*)\}\s*\}", text)
    assert len(rows) == 14
    out = []
    for r in rows:
        slots = [int(v, 16) for v in r[9].replace(" ", "").split(",") if v]
        assert len(slots) == 82
        out.append((int(r[0], 16), int(r[1]), int(r[2]), [int(v) for v in r[3:6]], [int(v) for v in r[6:9]], slots))
    return out


def _table(name):
    text = open(os.path.join(ROOT, "oracle", "bc7_tables.h")).read()
    body = re.search(name + r"\[128\]\s*=\s*\{([^}]*)\}", text).group(1)
    return np.array([int(v.rstrip("u"), 16) for v in re.findall(r"0x[0-9A-Fa-f]+u?", body)], dtype=np.int64)


LAYOUTS = _layouts()
PATTERN, ANCHORS = _table("BCN_PATTERN"), _table("BCN_ANCHORS")


# ---- the numpy decoder -------------------------------------------------------------------------------------------------------------------

def _sx(x, nb):
    """SIGN_EXTEND(x, nb): bit nb - 1 of an nb-bit field is its sign; nb a scalar or one value per channel."""
    nb = np.asarray(nb, dtype=np.int64)
    return np.where(x & (1 << (nb - 1)), x - (1 << nb), x)


def model(blocks, signed=True):
    """blocks -> dict: texels (n, 16, 4) uint16; modes (n,) int32, -1 reserved; and per block, of the endpoints the block uses:
    saturated (an endpoint unquantised to +-0x7FFF), wrapped (TransformInverse's mask changed a sum), negative (a sign bit set after the
    transform), neg_inf (a texel is 0xFC00).  signed=False is the unsigned reading (D3DXDecodeBC6HU), the flags then by its own rules."""
    b = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, 16)
    n = b.shape[0]
    bits = np.unpackbits(b, axis=1, bitorder="little").astype(np.int64)          # bit p of the 128, LSB first
    low5 = (bits[:, :5] << np.arange(5)).sum(axis=1)
    prefix = np.where((low5 & 3) < 2, low5 & 3, low5)
    modes = np.full(n, -1, dtype=np.int32)
    texels = np.zeros((n, 16, 4), dtype=np.uint16)
    texels[..., 3] = 0x3C00
    flags = {k: np.zeros(n, dtype=bool) for k in ("saturated", "wrapped", "negative", "neg_inf")}
    for mode, (pre, two, transformed, base, delta, slot) in enumerate(LAYOUTS):
        sel = np.nonzero(prefix == pre)[0]
        if not sel.size: continue
        modes[sel] = mode
        bb = bits[sel]
        m = sel.size
        header, ne, ib = (82, 4, 3) if two else (65, 2, 4)
        e = np.zeros((m, 4, 3), dtype=np.int64)
        shape = np.zeros(m, dtype=np.int64)
        for pos in range(header):
            field, bit = slot[pos] >> 4, slot[pos] & 15
            if field == 2: shape |= bb[:, pos] << bit
            elif field >= 3: e[:, (field - 3) & 3, (field - 3) >> 2] |= bb[:, pos] << bit
        base, delta = np.array(base), np.array(delta)
        wrapped = np.zeros(m, dtype=bool)
        if signed: e[:, 0] = _sx(e[:, 0], base)                                   # step 1
        if signed or transformed:
            for k in range(1, ne): e[:, k] = _sx(e[:, k], delta)
        if transformed:                                                           # step 2
            for k in range(1, ne):
                total = e[:, k] + e[:, 0]
                masked = total & ((1 << base) - 1)
                e[:, k] = _sx(masked, base) if signed else masked
                wrapped |= (e[:, k] != total).any(axis=1)
        used = e[:, :ne]
        if signed:                                                                # step 3
            mag = np.abs(e)
            top = (1 << (base - 1)) - 1
            sat = (mag >= top) & (base < 16)
            u = np.where(mag == 0, 0, np.where(mag >= top, 0x7FFF, ((mag << 15) + 0x4000) >> (base - 1)))
            unq = np.where(base >= 16, e, np.where(e < 0, -u, u))
        else:
            top = (1 << base) - 1
            sat = (e == top) & (base < 15)
            unq = np.where(base >= 15, e, np.where(e == 0, 0, np.where(e == top, 0xFFFF, ((e << 16) + 0x8000) >> base)))
        pattern = PATTERN[shape] if two else np.zeros(m, dtype=np.int64)
        anchor = (ANCHORS[shape] >> 4) if two else np.full(m, -1, dtype=np.int64)
        pos = np.full(m, header, dtype=np.int64)
        rows = np.arange(m)
        for k in range(16):
            region = (pattern >> (2 * k)) & 3
            nb = ib - ((k == 0) | ((region == 1) & (anchor == k))).astype(np.int64)
            idx = np.zeros(m, dtype=np.int64)
            for j in range(ib):
                idx |= np.where(j < nb, bb[rows, np.minimum(pos + j, 127)], 0) << j
            pos += nb
            w = (W3 if two else W4)[idx][:, None]
            a = np.where(region[:, None] == 1, unq[:, 2], unq[:, 0])
            c = np.where(region[:, None] == 1, unq[:, 3], unq[:, 1])
            x = (a * (64 - w) + c * w + 32) >> 6                                   # step 4: an arithmetic shift
            if signed:                                                            # steps 5 and 6
                mag = (np.abs(x) * 31) >> 5                                       # FinishUnquantize gives -mag, and -0 is 0:
                h = np.where((x < 0) & (mag != 0), 0x8000 | mag, mag)             # INT2F16 sees no sign on a zero
            else:
                h = np.minimum((x * 31) >> 6, 0x7BFF)
            texels[sel, k, :3] = h.astype(np.uint16)
        assert (pos == 128).all()
        flags["saturated"][sel] = sat[:, :ne].any(axis=(1, 2))
        flags["wrapped"][sel] = wrapped
        flags["negative"][sel] = (used < 0).any(axis=(1, 2)) if signed else False
        flags["neg_inf"][sel] = (texels[sel, :, :3] == 0xFC00).any(axis=(1, 2))
    return dict(texels=texels, modes=modes, **flags)


# ---- building blocks ---------------------------------------------------------------------------------------------------------------------

def pack_block(mode, shape, endpoints, indices):
    """A 128-bit word of `mode`: endpoints[4][3] raw field values (two's complement at the field's width; extra bits are dropped), shape
    0..31, indices[16] (a fix-up texel drops its top bit)."""
    pre, two, _, _, _, slot = LAYOUTS[mode]
    header, ib = (82, 3) if two else (65, 4)
    word = 0
    for pos in range(header):
        field, bit = slot[pos] >> 4, slot[pos] & 15
        v = pre if field == 1 else shape if field == 2 else int(endpoints[(field - 3) & 3][(field - 3) >> 2]) if field >= 3 else 0
        word |= ((v >> bit) & 1) << pos
    pos = header
    anchor = int(ANCHORS[shape]) >> 4 if two else -1
    for k in range(16):
        region = (int(PATTERN[shape]) >> (2 * k)) & 3 if two else 0
        nb = ib - (1 if k == 0 or (region == 1 and k == anchor) else 0)
        word |= (int(indices[k]) & ((1 << nb) - 1)) << pos
        pos += nb
    assert pos == 128
    return word


def constructed_blocks():
    """Set (b): per mode every pair (value of endpoint 0.A's fields, value of the other endpoints' fields) from 0, +-1, +-((1 << (bits - 1))
    - 1) and -(1 << (bits - 1)) at each field's own width, the channels rotated through the six values, each pair with indices all 0, all
    ones and a ramp.  In the transformed modes the pairs (largest, largest) and (most negative, most negative) wrap through the mask in
    either direction; in mode 13 a base of 0x8000 with delta 0 puts both endpoints at -32768, with any other delta one only."""
    def values(nb):
        top = (1 << (nb - 1)) - 1
        return [0, 1, -1, top, -top, -(1 << (nb - 1))]
    words = []
    for mode, (_, two, _, base, delta, _) in enumerate(LAYOUTS):
        for i in range(6):
            for j in range(6):
                e = [[0] * 3 for _ in range(4)]
                for ch in range(3):
                    e[0][ch] = values(base[ch])[(i + ch) % 6]
                    for k in range(1, 4):
                        e[k][ch] = values(delta[ch])[(j + ch * (k - 1)) % 6]
                for t, idx in enumerate(([0] * 16, [15] * 16, list(range(16)))):
                    words.append(pack_block(mode, (7 * (6 * i + j) + t) % 32 if two else 0, e, idx))
    return S._pack(words)


def random_blocks():
    """Set (c): 4 096 random 128-bit words."""
    return np.random.default_rng(SEED).integers(0, 256, 4096 * 16, dtype=np.uint8)


def sweep_blocks():
    """Set (a): the 8 192 blocks of _block_sweep.bc6h(), 256 x 512 texels; the same bytes give a signed stream."""
    return S.bc6h()[0]


def hdr_surface():
    """Set (d)'s source: 64 x 64 float RGB of both signs whose blocks straddle 0, (64, 64, 3) float32 (half-representable)."""
    rng = np.random.default_rng(SEED + 1)
    y, x = np.mgrid[0:64, 0:64].astype(np.float32)
    img = np.stack([np.sin(x / 5.0) * 3.0, (y - 32.0) / 8.0 + np.cos(x / 3.0), (x - y) / 16.0], axis=-1)
    img[32:, :32] *= 100.0
    img[:16, 48:] = np.abs(img[:16, 48:])
    img += rng.normal(0, 0.05, img.shape)
    return img.astype(np.float16).astype(np.float32)


def blocks_of(img):
    """(H, W, C) -> (H/4 * W/4, 16, C): the 16 texels of each block in raster order."""
    h, w, c = img.shape
    return img.reshape(h // 4, 4, w // 4, 4, c).transpose(0, 2, 1, 3, 4).reshape(-1, 16, c)


def image_of(texels, width, height):
    """(n, 16, C) texels of width/4 x height/4 blocks -> (height, width, C)."""
    c = texels.shape[-1]
    return texels.reshape(height // 4, width // 4, 4, 4, c).transpose(0, 2, 1, 3, 4).reshape(height, width, c)


def code(h):
    """A half bit pattern -> the integer the signed reading interpolates in (include/itw_decode.h): sign and magnitude, both zeros 0."""
    h = np.asarray(h).astype(np.int64)
    return np.where(h & 0x8000, -(h & 0x7FFF), h & 0x7FFF)


# ---- the reference ----------------------------------------------------------------------------------------------------------------------

def _aligned(shape, dtype):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.zeros(n + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 64
    return raw[off:off + n].view(dtype).reshape(shape)


def lib():
    L = B.lib()
    d = getattr(L, _DEC)
    d.argtypes = [C.c_void_p, C.c_void_p]
    d.restype = None
    e = getattr(L, _ENC)
    e.argtypes = [C.c_void_p, C.c_void_p, C.c_ulong]
    e.restype = None
    return L


def float_to_half_bits(f):
    """Floats widened from halves -> their half bits, exactly (asserted: the round trip gives the floats back, +-Inf included)."""
    f = np.asarray(f, dtype=np.float32)
    with np.errstate(over="ignore"):
        h = f.astype(np.float16)
    assert (h.astype(np.float32).view(np.uint32) == f.view(np.uint32)).all(), "a decoded float is not a half"
    return h.view(np.uint16)


def reference_decode(blocks):
    """blocks -> (n, 16, 4) uint16 through the reference's D3DXDecodeBC6HS."""
    fn = getattr(lib(), _DEC)
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, 16)
    n = blocks.shape[0]
    out = _aligned((n, 16, 4), np.float32)
    p, o = blocks.ctypes.data, out.ctypes.data
    for i in range(n):
        fn(o + i * 256, p + i * 16)
    return float_to_half_bits(np.array(out))


def reference_encode(img):
    """(H, W, 3) float32, H and W multiples of 4 -> the reference's D3DXEncodeBC6HS stream, flat uint8."""
    fn = getattr(lib(), _ENC)
    t = blocks_of(np.asarray(img, dtype=np.float32))
    n = t.shape[0]
    px = _aligned((n, 16, 4), np.float32)
    px[..., :3] = t
    px[..., 3] = 1.0
    out = np.zeros((n, 16), dtype=np.uint8)
    for i in range(n):
        fn(out.ctypes.data + i * 16, px.ctypes.data + i * 256, 0)
    return out.reshape(-1)


def golden():
    return np.load(GOLDEN)


def recorded_sets(g=None):
    """[(name, blocks flat uint8, texels (n, 16, 3) uint16)] of the recording: sweep, constructed, random and, if recorded, encoded."""
    g = g or golden()
    sets = [("sweep", sweep_blocks(), g["sweep_rgb"]), ("constructed", g["constructed_blocks"], g["constructed_rgb"]),
            ("random", g["random_blocks"], g["random_rgb"])]
    if "encoded_blocks" in g.files: sets.append(("encoded", g["encoded_blocks"], g["encoded_rgb"]))
    return sets
