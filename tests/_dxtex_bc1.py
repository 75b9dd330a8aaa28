"""The reference's BC1 codec with 1-bit alpha for the tests: D3DXEncodeBC1 / D3DXDecodeBC1 of oracle/_ref/libdxtex_bc_ref.so (BC.cpp compiled
unmodified by oracle/ref_build/Makefile), bound by their C++ names as tests/_dxtex_snorm.py binds the signed codecs; a numpy model of the
encoder (fp32, one rounding per operation, vectorised over blocks) that also says which branches of the source each block took; the content
the CPU and GPU tests share; and the recorded streams of tests/golden/bc1a_ref.npz (tools/gen_golden_bc1a.py).

Texel conversion (include/itw_dispatch.h): an RGBA8 code v is the float (float)v * (1.0f / 255.0f).  Partial blocks are filled as
DirectXTexCompress.cpp:140-168 fills them (_dxtex_snorm.block_texels)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from _dxtex_snorm import LIB, ROOT, _aligned, _boundary_heavy, block_texels

GOLDEN = os.path.join(ROOT, "tests", "golden", "bc1a_ref.npz")
DITHER_RGB, DITHER_A, UNIFORM = 0x10000, 0x20000, 0x40000
FLAG_SETS = tuple(r | a | u for u in (0, UNIFORM) for a in (0, DITHER_A) for r in (0, DITHER_RGB))        # the 8 combinations
F = np.float32
ALPHA_REFS = (F(0.0), F(0.5), F(128) * (F(1.0) / F(255.0)), F(1.0), F(1.5))
_ENC = "_ZN7DirectX13D3DXEncodeBC1EPhPKNS_8XMVECTOREfm"
_DEC = "_ZN7DirectX13D3DXDecodeBC1EPNS_8XMVECTOREPKh"
_lib = None


def lib():
    """The bound library; skips the calling test where it is absent and cannot be built (the golden streams are compared either way)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            if not os.path.exists("/root/reference/3rdParty/DirectXTex/DirectXTex/BC.cpp"):
                pytest.skip("oracle/_ref/libdxtex_bc_ref.so not prebuilt and /root/reference absent")
            subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True)
            subprocess.run(["make", "-C", os.path.join(ROOT, "oracle", "ref_build")], check=True)
        L = C.CDLL(LIB)
        e = getattr(L, _ENC)
        e.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_ulong]
        e.restype = None
        d = getattr(L, _DEC)
        d.argtypes = [C.c_void_p, C.c_void_p]
        d.restype = None
        _lib = L
    return _lib


def to_float(codes):
    return np.asarray(codes, dtype=np.uint8).astype(F) * (F(1.0) / F(255.0))


def encode_blocks(texels, alpha_ref, flags):
    """texels (n, 16, 4) uint8 -> (n, 8) uint8 through the reference's D3DXEncodeBC1."""
    fn = getattr(lib(), _ENC)
    texels = np.asarray(texels)
    assert texels.dtype == np.uint8 and texels.shape[1:] == (16, 4)
    n = texels.shape[0]
    px = _aligned((n, 16, 4), np.float32)
    px[...] = to_float(texels)
    out = np.zeros((n, 8), dtype=np.uint8)
    p, o = px.ctypes.data, out.ctypes.data
    for i in range(n):
        fn(o + i * 8, p + i * 256, float(alpha_ref), int(flags))
    return out


def encode(img, alpha_ref=0.5, flags=0):
    """The stream DirectX::Compress gives an RGBA8 image of any size: (H, W, 4) uint8 -> uint8 blocks, flat."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    return encode_blocks(block_texels(img), alpha_ref, flags).reshape(-1)


def decode(blocks):
    """blocks -> (n, 16, 4) float32, the reference's D3DXDecodeBC1."""
    fn = getattr(lib(), _DEC)
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, 8)
    n = blocks.shape[0]
    out = _aligned((n, 16, 4), np.float32)
    p, o = blocks.ctypes.data, out.ctypes.data
    for i in range(n):
        fn(o + i * 256, p + i * 8)
    return np.array(out)


# ---- content ------------------------------------------------------------------------------------------------------------------------

def boundary_heavy():
    """(128, 128, 4) uint8, 1 024 blocks: many exact 0 / 255 texels (alpha included), flat, collapsing and two-level blocks."""
    return _boundary_heavy(128, 128, 45)


def strip():
    """(32, 128, 4) uint8, 256 constructed blocks for the branches boundary_heavy() does not reach: nearly flat blocks one or two 5:6:5 steps
    wide (the two-colour return, Newton's exit by length, equal endpoints in a 3-step block), smooth ramps (Newton running long), two
    clusters (the epsilon exit), each with opaque, cut-out and mid-grey alpha (what alpha dithering turns around)."""
    rng = np.random.default_rng(1883)
    blocks = np.zeros((256, 16, 4), dtype=np.uint8)
    ramp = np.arange(16)
    for b in range(256):
        family, alpha_kind = b % 8, (b // 8) % 4
        base = rng.integers(0, 256, 3)
        if family == 0:                                    # one channel one or two codes of 5 bits apart, the rest flat
            t = np.tile(base, (16, 1))
            ch = rng.integers(0, 3)
            t[:, ch] = np.clip(base[ch] + rng.integers(0, 2, 16) * rng.integers(4, 17), 0, 255)
        elif family == 1:                                  # nearly flat: noise of a few codes
            t = np.clip(base[None, :] + rng.integers(-3, 4, (16, 3)), 0, 255)
        elif family == 2:                                  # a smooth ramp between two colours
            other = rng.integers(0, 256, 3)
            t = (base[None, :] * (15 - ramp)[:, None] + other[None, :] * ramp[:, None]) // 15
        elif family == 3:                                  # two clusters
            other = rng.integers(0, 256, 3)
            t = np.where(rng.integers(0, 2, 16)[:, None] == 1, base[None, :], other[None, :]) + rng.integers(-2, 3, (16, 3))
            t = np.clip(t, 0, 255)
        elif family == 4:                                  # dark, short ramps (endpoints that quantise to one 5:6:5 word)
            t = np.clip((base[None, :] // 16) + (ramp[:, None] * rng.integers(0, 3, 3)[None, :]) // 4, 0, 255)
        elif family == 5:                                  # bright with a few outliers
            t = np.clip(240 + rng.integers(-8, 16, (16, 3)), 0, 255)
            t[rng.integers(0, 16, 2)] = rng.integers(0, 256, (2, 3))
        elif family == 6:                                  # one colour exactly
            t = np.tile(base, (16, 1))
        else:                                              # noise
            t = rng.integers(0, 256, (16, 3))
        if alpha_kind == 0:
            a = np.full(16, 255)
        elif alpha_kind == 1:
            a = np.where(rng.integers(0, 4, 16) == 0, 0, 255)
        elif alpha_kind == 2:
            a = rng.integers(96, 160, 16)                  # around every alpha_ref the tests use but the extremes
        else:
            a = rng.integers(0, 256, 16)
        blocks[b, :, :3] = t
        blocks[b, :, 3] = a
    # Newton's exit by length (the endpoints converge below 1/4096 after the first step): a flat block with two near outliers
    flat = np.tile(np.array([114, 89, 41, 255], dtype=np.uint8), (16, 1))
    flat[8, :3] = (121, 88, 30)
    flat[14, :3] = (113, 90, 65)
    blocks[6] = flat
    return np.ascontiguousarray(blocks.reshape(8, 32, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(32, 128, 4))


def content():
    """name -> image: what the CPU model test, the golden file and the GPU tests all encode."""
    return {"boundary": boundary_heavy(), "strip": strip()}


def golden_key(name, alpha_ref, flags):
    return "%s.%08x.%05x" % (name, int(np.float32(alpha_ref).view(np.uint32)), flags)


_golden = None


def golden():
    """The reference's recorded streams (tools/gen_golden_bc1a.py): golden_key(...) -> uint8 stream.  A missing file fails the caller."""
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


# ---- the model: D3DXEncodeBC1 -> EncodeBC1(bColorKey = true) -> OptimizeRGB (BC.cpp:67-318, 372-677, 729-787) in numpy ---------------------

PATHS = ("all_transparent", "steps3", "steps4", "flt_min_return", "two_colour_return", "newton_exit_length", "newton_exit_epsilon",
         "newton_all_8", "solid_return", "steps3_equal_endpoints", "order_kept", "order_swapped")
DITHER_A_PATHS = ("dither_a_key_changed", "dither_a_rounded_up", "dither_a_rounded_down")
# (No path for "dithering made a value negative before static_cast<int32_t>": a texel's error is a convex combination of differences of at
# most half a quantisation step, so code 0 plus its error plus the rounding half never falls below zero, for colour and alpha alike.)
DITHER_RGB_PATHS = ("dither_rgb_quant_changed", "dither_rgb_transparent_skipped", "dither_rgb_index_changed")


def _diffuse(E, i, d, mask=None):
    """Floyd-Steinberg inside the block: E (n, 16[, 3]) += texel i's difference d, to the right, lower left, below, lower right."""
    def add(j, wgt):
        v = E[:, j] + d * F(wgt)
        E[:, j] = v if mask is None else np.where(mask if v.ndim == 1 else mask[:, None], v, E[:, j])
    if (i & 3) != 3:
        add(i + 1, 7.0 / 16.0)
    if i < 12:
        if i & 3:
            add(i + 3, 3.0 / 16.0)
        add(i + 4, 5.0 / 16.0)
        if (i & 3) != 3:
            add(i + 5, 1.0 / 16.0)


def _trunc(x):
    return np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0).astype(np.int32)        # static_cast<int32_t>: toward zero


def model(texels, alpha_ref, flags):
    """texels (n, 16, 4) uint8 -> ((n, 8) uint8 blocks, {path name: (n,) bool}).  Every operation is one fp32 operation of the source, in
    its order; a block that returned early carries garbage through the later stages, which its masks discard."""
    texels = np.asarray(texels)
    n = texels.shape[0]
    t = to_float(texels)
    aref = F(alpha_ref)
    drgb, da, uni = bool(flags & DITHER_RGB), bool(flags & DITHER_A), bool(flags & UNIFORM)
    paths = {}
    with np.errstate(all="ignore"):
        # D3DXEncodeBC1: the alpha the key test sees
        a = t[..., 3]
        if da:
            E = np.zeros((n, 16), dtype=F)
            A = np.empty((n, 16), dtype=F)
            for i in range(16):
                alph = a[:, i] + E[:, i]
                q = _trunc(alph + F(0.5)).astype(F)
                A[:, i] = q
                _diffuse(E, i, alph - q)
            paths["dither_a_key_changed"] = ((A < aref) != (a < aref)).any(axis=1)
            paths["dither_a_rounded_up"] = (A > a).any(axis=1)
            paths["dither_a_rounded_down"] = (A < a).any(axis=1)
            a = A
        key = a < aref
        nkey = key.sum(axis=1)
        all_t = nkey == 16
        three = (nkey > 0) & ~all_t
        live = ~all_t
        paths["all_transparent"] = all_t
        paths["steps3"] = three
        paths["steps4"] = live & ~three

        lum = np.array([1.0, 1.0, 1.0], dtype=F) if uni else np.array([F(0.2125) / F(0.7154), F(1.0), F(0.0721) / F(0.7154)], dtype=F)
        inv = np.array([1.0, 1.0, 1.0], dtype=F) if uni else np.array([F(0.7154) / F(0.2125), F(1.0), F(0.7154) / F(0.0721)], dtype=F)
        scale = np.array([31.0, 63.0, 31.0], dtype=F)
        iscale = np.array([F(1.0) / F(31.0), F(1.0) / F(63.0), F(1.0) / F(31.0)], dtype=F)
        col = t[..., :3]

        # EncodeBC1, first pass: quantise to 5:6:5
        P = np.empty((n, 16, 3), dtype=F)
        E = np.zeros((n, 16, 3), dtype=F)
        changed = np.zeros(n, dtype=bool)
        for i in range(16):
            clr = col[:, i] + E[:, i] if drgb else col[:, i]
            qi = _trunc(clr * scale + F(0.5))
            c = qi.astype(F) * iscale
            if drgb:
                changed |= (qi != _trunc(col[:, i] * scale + F(0.5))).any(axis=1)
                _diffuse(E, i, clr - c)
            P[:, i] = c * lum
        if drgb:
            paths["dither_rgb_quant_changed"] = changed & live

        # OptimizeRGB
        fsteps = np.where(three, F(2.0), F(3.0)).astype(F)
        last = np.where(three, 2, 3)
        Cw = np.where(three[:, None], np.array([F(2.0) / F(2.0), F(1.0) / F(2.0), F(0.0) / F(2.0), F(0.0)], dtype=F)[None, :],
                      np.array([F(3.0) / F(3.0), F(2.0) / F(3.0), F(1.0) / F(3.0), F(0.0) / F(3.0)], dtype=F)[None, :]).astype(F)
        Dw = np.where(three[:, None], np.array([F(0.0) / F(2.0), F(1.0) / F(2.0), F(2.0) / F(2.0), F(1.0)], dtype=F)[None, :],
                      np.array([F(0.0) / F(3.0), F(1.0) / F(3.0), F(2.0) / F(3.0), F(3.0) / F(3.0)], dtype=F)[None, :]).astype(F)
        X = np.tile(lum, (n, 1))
        Y = np.zeros((n, 3), dtype=F)
        for i in range(16):
            X = np.where(P[:, i] < X, P[:, i], X)
            Y = np.where(P[:, i] > Y, P[:, i], Y)
        AB = Y - X
        fAB = AB[:, 0] * AB[:, 0] + AB[:, 1] * AB[:, 1] + AB[:, 2] * AB[:, 2]
        flt_min = fAB < np.finfo(F).tiny
        paths["flt_min_return"] = live & flt_min
        go = ~flt_min
        fABinv = F(1.0) / fAB
        Dir = AB * fABinv[:, None]
        Mid = (X + Y) * F(0.5)
        fDir = np.zeros((n, 4), dtype=F)
        for i in range(16):
            pt = (P[:, i] - Mid) * Dir
            for k, (sg, sb) in enumerate(((1, 1), (1, -1), (-1, 1), (-1, -1))):
                f = (pt[:, 0] + pt[:, 1] if sg > 0 else pt[:, 0] - pt[:, 1])
                f = f + pt[:, 2] if sb > 0 else f - pt[:, 2]
                fDir[:, k] = fDir[:, k] + f * f
        fmax = fDir[:, 0].copy()
        imax = np.zeros(n, dtype=np.int64)
        for k in range(1, 4):
            better = fDir[:, k] > fmax
            fmax = np.where(better, fDir[:, k], fmax)
            imax = np.where(better, k, imax)
        swap_g = go & ((imax & 2) != 0)
        swap_b = go & ((imax & 1) != 0)
        Xg, Yg = np.where(swap_g, Y[:, 1], X[:, 1]), np.where(swap_g, X[:, 1], Y[:, 1])
        Xb, Yb = np.where(swap_b, Y[:, 2], X[:, 2]), np.where(swap_b, X[:, 2], Y[:, 2])
        X = np.stack([X[:, 0], Xg, Xb], axis=1)
        Y = np.stack([Y[:, 0], Yg, Yb], axis=1)
        two = go & (fAB < F(1.0) / F(4096.0))
        paths["two_colour_return"] = live & two
        active = go & ~two
        eps = (F(0.25) / F(64.0)) * (F(0.25) / F(64.0))
        exit_len = np.zeros(n, dtype=bool)
        exit_eps = np.zeros(n, dtype=bool)
        rows = np.arange(n)
        for _ in range(8):
            S = X[:, None, :] * Cw[:, :, None] + Y[:, None, :] * Dw[:, :, None]                 # pSteps (n, 4, 3)
            Dir = Y - X
            flen = Dir[:, 0] * Dir[:, 0] + Dir[:, 1] * Dir[:, 1] + Dir[:, 2] * Dir[:, 2]
            brk = active & (flen < F(1.0) / F(4096.0))
            exit_len |= brk
            active = active & ~brk
            Dir = Dir * (fsteps / flen)[:, None]
            d2X = np.zeros(n, dtype=F)
            d2Y = np.zeros(n, dtype=F)
            dX = np.zeros((n, 3), dtype=F)
            dY = np.zeros((n, 3), dtype=F)
            for i in range(16):
                df = P[:, i] - X
                dot = df[:, 0] * Dir[:, 0] + df[:, 1] * Dir[:, 1] + df[:, 2] * Dir[:, 2]
                k = np.where(dot <= 0, 0, np.where(dot >= fsteps, last, np.clip(_trunc(dot + F(0.5)), 0, 3)))
                pc, pd = Cw[rows, k], Dw[rows, k]
                diff = S[rows, k] - P[:, i]
                fc, fd = pc * (F(1.0) / F(8.0)), pd * (F(1.0) / F(8.0))
                d2X = d2X + fc * pc
                dX = dX + fc[:, None] * diff
                d2Y = d2Y + fd * pd
                dY = dY + fd[:, None] * diff
            mx = active & (d2X > 0)
            X = np.where(mx[:, None], X + dX * (F(-1.0) / d2X)[:, None], X)
            my = active & (d2Y > 0)
            Y = np.where(my[:, None], Y + dY * (F(-1.0) / d2Y)[:, None], Y)
            small = ((dX * dX < eps).all(axis=1)) & ((dY * dY < eps).all(axis=1))
            brk = active & small
            exit_eps |= brk
            active = active & ~brk
        paths["newton_exit_length"] = live & exit_len
        paths["newton_exit_epsilon"] = live & exit_eps
        paths["newton_all_8"] = live & active

        # EncodeBC1: the endpoints
        def encode565(c):
            c = np.where(c < 0, F(0.0), np.where(c > 1, F(1.0), c)).astype(F)
            q = _trunc(c * scale + F(0.5))
            return ((q[:, 0] << 11) | (q[:, 1] << 5) | q[:, 2]) & 0xFFFF

        def decode565(w):
            return np.stack([((w >> 11) & 31).astype(F), ((w >> 5) & 63).astype(F), (w & 31).astype(F)], axis=1) * iscale

        wa, wb = encode565(X * inv), encode565(Y * inv)
        solid = live & ~three & (wa == wb)
        paths["solid_return"] = solid
        rest = live & ~solid
        paths["steps3_equal_endpoints"] = rest & three & (wa == wb)
        A_, B_ = decode565(wa) * lum, decode565(wb) * lum
        ab = three == (wa <= wb)
        paths["order_kept"] = rest & ab
        paths["order_swapped"] = rest & ~ab
        e0, e1 = np.where(ab, wa, wb), np.where(ab, wb, wa)
        T0, T1 = np.where(ab[:, None], A_, B_), np.where(ab[:, None], B_, A_)
        T2 = T0 + np.where(three, F(0.5), F(1.0) / F(3.0)).astype(F)[:, None] * (T1 - T0)
        T3 = T0 + (F(2.0) / F(3.0)) * (T1 - T0)
        T = np.stack([T0, T1, T2, T3], axis=1)
        Dir = T1 - T0
        den = Dir[:, 0] * Dir[:, 0] + Dir[:, 1] * Dir[:, 1] + Dir[:, 2] * Dir[:, 2]
        fscale = np.where(wa != wb, fsteps / den, F(0.0)).astype(F)
        Dir = Dir * fscale[:, None]

        # EncodeBC1: the indices
        def indices(dither):
            dw = np.zeros(n, dtype=np.uint64)
            E = np.zeros((n, 16, 3), dtype=F)
            skipped = np.zeros(n, dtype=bool)
            order = np.where(three[:, None], np.array([0, 2, 1, 1])[None, :], np.array([0, 2, 3, 1])[None, :])      # pSteps3 / pSteps4
            for i in range(16):
                skip = three & key[:, i]
                clr = col[:, i] * lum
                if dither:
                    clr = clr + E[:, i]
                df = clr - T0
                dot = df[:, 0] * Dir[:, 0] + df[:, 1] * Dir[:, 1] + df[:, 2] * Dir[:, 2]
                step = np.where(dot <= 0, 0, np.where(dot >= fsteps, 1, order[rows, np.clip(_trunc(dot + F(0.5)), 0, 3)]))
                step = np.where(skip, 3, step)
                dw = (step.astype(np.uint64) << np.uint64(30)) | (dw >> np.uint64(2))
                if dither:
                    skipped |= skip
                    _diffuse(E, i, clr - T[rows, step], ~skip)
            return dw, skipped

        dw, skipped = indices(drgb)
        if drgb:
            paths["dither_rgb_transparent_skipped"] = rest & skipped
            paths["dither_rgb_index_changed"] = rest & (indices(False)[0] != dw)

    ends = (e0 | (e1 << 16)).astype(np.uint32)
    bitmap = dw.astype(np.uint32)
    ends = np.where(solid, (wa | (wb << 16)).astype(np.uint32), ends)
    bitmap = np.where(solid, np.uint32(0), bitmap)
    ends = np.where(all_t, np.uint32(0xFFFF0000), ends)
    bitmap = np.where(all_t, np.uint32(0xFFFFFFFF), bitmap)
    out = np.stack([ends.astype("<u4"), bitmap.astype("<u4")], axis=1)
    return np.ascontiguousarray(out).view(np.uint8).reshape(n, 8), paths


def census(paths):
    return {k: int(v.sum()) for k, v in paths.items()}


# ---- the kernel's text on the host (tools/bc1a_host_check.cpp over csrc/bc1a_core.hpp) -----------------------------------------------------

def build_host_check(tmp_dir):
    exe = os.path.join(str(tmp_dir), "bc1a_host_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "bc1a_host_check.cpp"), "-o", exe], check=True)
    return exe


def host_check_encode(exe, tmp_dir, texels, alpha_ref, flags):
    src, dst = os.path.join(str(tmp_dir), "texels.bin"), os.path.join(str(tmp_dir), "blocks.bin")
    np.ascontiguousarray(texels, dtype=np.uint8).tofile(src)
    subprocess.run([exe, src, dst, "%08x" % int(np.float32(alpha_ref).view(np.uint32)), str(flags)], check=True)
    return np.fromfile(dst, dtype=np.uint8).reshape(-1, 8)
