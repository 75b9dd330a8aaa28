"""The reference's BC3 encoder for the tests: D3DXEncodeBC3 of oracle/_ref/libdxtex_bc_ref.so (BC.cpp compiled unmodified by
oracle/ref_build/Makefile), bound by its C++ name as tests/_dxtex_bc2.py binds the BC2 pair; a numpy model of the encoder's alpha half
(BC.cpp:952-1003, 1018-1138 with OptimizeAlpha<false>, BC.h:727-856: fp32, one rounding per operation, vectorised over blocks) that also
names, per block, the branches it took -- the colour half is _dxtex_bc1.model with alpha_ref 0 and without DITHER_A, which is what
D3DXEncodeBC3 calls; the content the CPU and GPU tests share; and the recorded streams of tests/golden/bc3_dxtex_ref.npz
(tools/gen_golden_bc3_dxtex.py).

Texel conversion (include/itw_dispatch.h): an RGBA8 code v is the float (float)v * (1.0f / 255.0f).  Partial blocks are filled as
DirectXTexCompress.cpp:140-168 fills them (_dxtex_snorm.block_texels)."""
import ctypes as C
import os
import subprocess

import numpy as np

import _dxtex_bc1 as B
from _dxtex_bc1 import DITHER_A, DITHER_RGB, FLAG_SETS, UNIFORM, F, _diffuse, _trunc, to_float      # noqa: F401
from _dxtex_bc2 import SIZE_FLAGS, SIZES, size_image, size_key                                       # noqa: F401  (the five odd sizes)
from _dxtex_snorm import ROOT, _aligned, block_texels

GOLDEN = os.path.join(ROOT, "tests", "golden", "bc3_dxtex_ref.npz")
_ENC = "_ZN7DirectX13D3DXEncodeBC3EPhPKNS_8XMVECTOREm"
_bound = False


def lib():
    """The bound library; skips the calling test where it is absent and cannot be built (the golden streams are compared either way)."""
    global _bound
    L = B.lib()
    if not _bound:
        e = getattr(L, _ENC)
        e.argtypes = [C.c_void_p, C.c_void_p, C.c_ulong]
        e.restype = None
        _bound = True
    return L


def encode_blocks(texels, flags):
    """texels (n, 16, 4) uint8 -> (n, 16) uint8 through the reference's D3DXEncodeBC3."""
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


# ---- content ------------------------------------------------------------------------------------------------------------------------

def alpha_blocks():
    """(16, 128, 4) uint8, 128 constructed blocks for what the alpha half of D3DXEncodeBC3 can do.  0..7 all opaque or all one value; 8..23
    a 0 among middle values (6 steps because of a 0; code 6; the `<= 0` branch staying at step 0); 24..39 a 255 among middle values (6 steps
    because of a 1; code 7; the `>= fSteps` branch staying at step 1); 40..47 both; 48..63 ramps and noise without 0 or 255 (8 steps; two
    neighbouring values: OptimizeAlpha ends at once by its width test); 64..71 a 254 or a 1 among near values (where a diffused point of the
    pre-pass would leave 0..1 if an RGBA8 source left it an error to diffuse: UNREACHED_BRANCHES below); the rest random.  Colour: noise
    (the colour half has its own content)."""
    rng = np.random.default_rng(3077)
    blocks = np.zeros((128, 16, 4), dtype=np.uint8)
    blocks[..., :3] = rng.integers(0, 256, (128, 16, 3))
    al = rng.integers(0, 256, (128, 16))
    for b, v in enumerate((255, 255, 0, 128, 1, 254, 77, 200)):
        al[b] = v
    al[1, 7] = 254
    for b in range(8, 24):
        lo, hi = sorted(int(v) for v in rng.integers(1, 255, 2))
        al[b] = rng.integers(lo, hi + 1, 16)
        al[b, rng.integers(0, 16, 1 + b % 5)] = 0
        if b % 4 == 0:
            al[b, rng.integers(0, 16, 2)] = max(1, lo // 3)      # nearer to 0 than to the ramp's foot, but not 0
    for b in range(24, 40):
        lo, hi = sorted(int(v) for v in rng.integers(1, 255, 2))
        al[b] = rng.integers(lo, hi + 1, 16)
        al[b, rng.integers(0, 16, 1 + b % 5)] = 255
        if b % 4 == 0:
            al[b, rng.integers(0, 16, 2)] = min(254, hi + 2 * (255 - hi) // 3)
    for b in range(40, 48):
        lo, hi = sorted(int(v) for v in rng.integers(1, 255, 2))
        al[b] = rng.integers(lo, hi + 1, 16)
        al[b, rng.integers(0, 8, 2)] = 0
        al[b, rng.integers(8, 16, 2)] = 255
    al[46] = np.where(np.arange(16) % 2, 255, 0)
    al[47] = np.where(np.arange(16) % 3, 0, 90)
    for b in range(48, 56):
        al[b] = np.clip(10 + 30 * (b - 48) + (np.arange(16) * (1 + b % 3)), 1, 254)
    for b in range(56, 64):
        al[b] = rng.integers(1, 255, 16)
    al[56] = np.where(np.arange(16) < 8, 100, 101)
    al[57] = np.where(np.arange(16) < 15, 100, 102)
    for b in range(64, 68):
        al[b] = rng.integers(200, 255, 16)
        al[b, 5 + (b & 3)] = 254
    for b in range(68, 72):
        al[b] = rng.integers(1, 56, 16)
        al[b, 5 + (b & 3)] = 1
    blocks[..., 3] = al
    return np.ascontiguousarray(blocks.reshape(4, 32, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(16, 128, 4))


_content = None


def content():
    """name -> image: what the CPU model test, the golden file and the GPU tests all encode: _dxtex_bc1's shared content plus alpha_blocks()."""
    global _content
    if _content is None:
        _content = dict(B.content())
        _content["alpha"] = alpha_blocks()
    return _content


def golden_key(name, flags):
    return "%s.%05x" % (name, flags)


_golden = None


def golden():
    """The reference's recordings (tools/gen_golden_bc3_dxtex.py): golden_key(...) / size_key(...) -> uint8 stream.  A missing file fails the caller."""
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


# ---- the model: the alpha half of D3DXEncodeBC3 (BC.cpp:939-1139) in numpy ---------------------------------------------------------------

BRANCHES = ("all_opaque", "six_by_zero", "six_by_one", "eight", "eight_equal_endpoints", "six_equal_endpoints", "code_6", "code_7",
            "below_ramp_step_0", "above_ramp_step_1", "optimize_exit_width", "optimize_exit_epsilon", "optimize_all_8", "optimize_swap")
DITHER_A_BRANCHES = ("point_above_one", "point_below_zero", "steps_changed")
# Branches of the source that no RGBA8 block is known to take (DESIGN.md 3.18 gives the reasons); the model and the kernel restate them all the
# same, and test_bc3_dxtex_cpu.py asserts that the shared content does not take them, so a block that does would show.
#  * the three DITHER_A ones cannot be taken: a texel is (float)v * (1.0f / 255.0f), and (int32_t)(that * 255.0f + 0.5f) * (1.0f / 255.0f) is
#    the same float for every v in 0..255 (prepass_is_identity() walks them), so the pre-pass never has an error to diffuse: its points are
#    the source alphas, with the flag or without.
#  * six_equal_endpoints, optimize_all_8, optimize_swap: none in 1.7 million searched blocks (levels, clusters beside a 0 or a 255, ramps,
#    noise); the 6-step start values are two different codes or (x, 1), the fit keeps them apart, and a Newton step is a weighted mean of
#    residuals of at most half a step, far less than the ramp's width and, after one pass, than the 1/8 of the loop's exit test.
UNREACHED_BRANCHES = ("six_equal_endpoints", "optimize_all_8", "optimize_swap") + DITHER_A_BRANCHES


def prepass_is_identity():
    """True when the pre-pass rounds every RGBA8 alpha to itself in fp32 (so DITHER_A diffuses zeros there)."""
    a = to_float(np.arange(256, dtype=np.uint8))
    return bool(np.array_equal((_trunc(a * F(255.0) + F(0.5)).astype(F) * _INV255).view(np.uint32), a.view(np.uint32)))

_Q5 = np.array([5, 4, 3, 2, 1, 0, 0, 0], dtype=F) / F(5.0)
_Q7 = np.array([7, 6, 5, 4, 3, 2, 1, 0], dtype=F) / F(7.0)
_D5 = np.array([0, 1, 2, 3, 4, 5, 0, 0], dtype=F) / F(5.0)
_D7 = np.array([0, 1, 2, 3, 4, 5, 6, 7], dtype=F) / F(7.0)
_INV255 = F(1.0) / F(255.0)


def _prepass(a, da):
    """a (n, 16) fp32 alpha -> the points fAlpha[], fMinAlpha, fMaxAlpha."""
    n = a.shape[0]
    pt = np.zeros((n, 16), dtype=F)
    E = np.zeros((n, 16), dtype=F)
    fmin, fmax = a[:, 0].copy(), a[:, 0].copy()                     # Color[0].a, the unrounded value
    for i in range(16):
        alph = a[:, i] + E[:, i] if da else a[:, i]
        q = _trunc(alph * F(255.0) + F(0.5)).astype(F) * _INV255    # toward zero
        pt[:, i] = q
        lower = q < fmin
        higher = ~lower & (q > fmax)                                # `else if`
        fmin = np.where(lower, q, fmin)
        fmax = np.where(higher, q, fmax)
        if da:
            _diffuse(E, i, alph - q)
    return pt, fmin, fmax


def _optimize_alpha(pt, six):
    """OptimizeAlpha<false> over pt (n, 16) -> fX, fY (clamped) and how each block's loop ended."""
    n = pt.shape[0]
    rows = np.arange(n)
    c = np.where(six[:, None], _Q5, _Q7)
    d = np.where(six[:, None], _D5, _D7)
    fx, fy = np.ones(n, dtype=F), np.zeros(n, dtype=F)
    for i in range(16):
        p = pt[:, i]
        fx = np.where((p < fx) & (~six | (p > F(0.0))), p, fx)
        fy = np.where((p > fy) & (~six | (p < F(1.0))), p, fy)
    fy = np.where(six & (fx == fy), F(1.0), fy)
    fsteps = np.where(six, F(5.0), F(7.0)).astype(F)
    csteps = np.where(six, 6, 8)
    live = np.ones(n, dtype=bool)
    ends = {k: np.zeros(n, dtype=bool) for k in ("optimize_exit_width", "optimize_exit_epsilon", "optimize_all_8", "optimize_swap")}
    for _ in range(8):
        narrow = (fy - fx) < F(1.0 / 256.0)
        ends["optimize_exit_width"] |= live & narrow
        live = live & ~narrow
        scale = fsteps / (fy - fx)
        s = c * fx[:, None] + d * fy[:, None]
        to_zero, to_one = fx * F(0.5), (fy + F(1.0)) * F(0.5)
        dx, dy, d2x, d2y = (np.zeros(n, dtype=F) for _ in range(4))
        for i in range(16):
            p = pt[:, i]
            dot = (p - fx) * scale
            k = np.where(dot <= F(0.0), np.where(six & (p <= to_zero), 6, 0),
                         np.where(dot >= fsteps, np.where(six & (p >= to_one), 7, csteps - 1), _trunc(dot + F(0.5))))
            use = k < csteps
            kk = np.clip(k, 0, 7)
            ck, dk = c[rows, kk], d[rows, kk]
            diff = s[rows, kk] - p
            dx = np.where(use, dx + ck * diff, dx)
            d2x = np.where(use, d2x + ck * ck, d2x)
            dy = np.where(use, dy + dk * diff, dy)
            d2y = np.where(use, d2y + dk * dk, d2y)
        nx = np.where(d2x > F(0.0), fx - dx / d2x, fx)
        ny = np.where(d2y > F(0.0), fy - dy / d2y, fy)
        swap = nx > ny
        nx, ny = np.where(swap, ny, nx), np.where(swap, nx, ny)
        ends["optimize_swap"] |= live & swap
        fx, fy = np.where(live, nx, fx), np.where(live, ny, fy)
        done = (dx * dx < F(1.0 / 64.0)) & (dy * dy < F(1.0 / 64.0))
        ends["optimize_exit_epsilon"] |= live & done
        live = live & ~done
    ends["optimize_all_8"] = live
    return np.clip(fx, F(0.0), F(1.0)), np.clip(fy, F(0.0), F(1.0)), ends


def alpha_model(texels, flags):
    """texels (n, 16, 4) uint8 -> ((n, 8) uint8: alpha[0], alpha[1], bitmap[0..5], {branch: (n,) bool}).  A block that returned early
    carries garbage through the later stages, which its masks discard."""
    texels = np.asarray(texels)
    n = texels.shape[0]
    rows = np.arange(n)
    a = to_float(texels)[..., 3]
    da = bool(flags & DITHER_A)
    br = {k: np.zeros(n, dtype=bool) for k in BRANCHES + DITHER_A_BRANCHES}
    with np.errstate(all="ignore"):
        pt, fmin, fmax = _prepass(a, da)
        opaque = fmin == F(1.0)
        six = (fmin == F(0.0)) | (fmax == F(1.0))
        run = ~opaque
        fa, fb, ends = _optimize_alpha(pt, six)
        ba = (_trunc(fa * F(255.0) + F(0.5)) & 0xFF).astype(np.uint32)
        bb = (_trunc(fb * F(255.0) + F(0.5)) & 0xFF).astype(np.uint32)
        fa, fb = ba.astype(F) * _INV255, bb.astype(F) * _INV255
        equal8 = run & ~six & (ba == bb)
        idx = run & ~equal8                                          # the blocks that reach the index pass
        st = np.zeros((n, 8), dtype=F)
        st[:, 0] = np.where(six, fa, fb)
        st[:, 1] = np.where(six, fb, fa)
        e0 = np.where(six, ba, bb)
        e1 = np.where(six, bb, ba)
        for i in range(1, 7):
            v8 = (st[:, 0] * F(7 - i) + st[:, 1] * F(i)) * (F(1.0) / F(7.0))
            v6 = (st[:, 0] * F(5 - i) + st[:, 1] * F(i)) * (F(1.0) / F(5.0)) if i < 5 else np.full(n, F(0.0) if i == 5 else F(1.0))
            st[:, i + 1] = np.where(six, v6, v8)
        fsteps = np.where(six, F(5.0), F(7.0)).astype(F)
        last = np.where(six, 5, 7)
        scale = np.where(st[:, 0] != st[:, 1], fsteps / (st[:, 1] - st[:, 0]), F(0.0)).astype(F)
        to_zero, to_one = st[:, 0] * F(0.5), (st[:, 1] + F(1.0)) * F(0.5)
        E = np.zeros((n, 16), dtype=F)
        dw = np.zeros((n, 2), dtype=np.uint32)
        for i in range(16):
            alph = a[:, i] + E[:, i] if da else a[:, i]
            dot = (alph - st[:, 0]) * scale
            below, above = dot <= F(0.0), ~(dot <= F(0.0)) & (dot >= fsteps)
            k = _trunc(dot + F(0.5))
            mid = np.where(k == 0, 0, np.where(k == last, 1, k + 1))
            step = np.where(below, np.where(six & (alph <= to_zero), 6, 0), np.where(above, np.where(six & (alph >= to_one), 7, 1), mid))
            step = np.clip(step, 0, 7).astype(np.uint32)
            dw[:, i >> 3] = (step << np.uint32(21)) | (dw[:, i >> 3] >> np.uint32(3))
            br["code_6"] |= idx & (step == 6)
            br["code_7"] |= idx & (step == 7)
            br["below_ramp_step_0"] |= idx & six & below & (step == 0)
            br["above_ramp_step_1"] |= idx & six & above & (step == 1)
            if da:
                _diffuse(E, i, alph - st[rows, step])
        w0 = e0 | (e1 << np.uint32(8)) | ((dw[:, 0] & np.uint32(0xFFFF)) << np.uint32(16))
        w1 = ((dw[:, 0] >> np.uint32(16)) & np.uint32(0xFF)) | (dw[:, 1] << np.uint32(8))
        w0 = np.where(opaque, np.uint32(0xFFFF), np.where(equal8, ba | (bb << np.uint32(8)), w0))
        w1 = np.where(opaque | equal8, np.uint32(0), w1)
        br["all_opaque"] = opaque
        br["six_by_zero"] = run & (fmin == F(0.0))
        br["six_by_one"] = run & (fmax == F(1.0))
        br["eight"] = run & ~six
        br["eight_equal_endpoints"] = equal8
        br["six_equal_endpoints"] = idx & six & (ba == bb)
        for k, v in ends.items():
            br[k] = run & v
        if da:
            _, pmin, pmax = _prepass(a, False)
            br["point_above_one"] = (pt > F(1.0)).any(axis=1)
            br["point_below_zero"] = (pt < F(0.0)).any(axis=1)
            br["steps_changed"] = run & (pmin != F(1.0)) & (six != ((pmin == F(0.0)) | (pmax == F(1.0))))
    out = np.stack([w0, w1], axis=1).astype("<u4")
    return np.ascontiguousarray(out).view(np.uint8).reshape(n, 8), br


def model(texels, flags):
    """texels (n, 16, 4) uint8 -> ((n, 16) uint8 blocks, branches of the alpha half, paths of the colour half)."""
    alpha, branches = alpha_model(texels, flags)
    colour, cpaths = B.model(texels, 0.0, flags & ~DITHER_A)          # EncodeBC1(..., false, 0.f, flags), which never reads DITHER_A
    return np.concatenate([alpha, colour], axis=1), branches, cpaths


def census(branches):
    return {k: int(v.sum()) for k, v in branches.items()}


# ---- the kernel's text on the host (tools/bc3_host_check.cpp over csrc/bc3_core.hpp) -----------------------------------------------------

def build_host_check(tmp_dir, extra=()):
    exe = os.path.join(str(tmp_dir), "bc3_host_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", *extra, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "bc3_host_check.cpp"), "-o", exe], check=True)
    return exe


def host_check_encode(exe, tmp_dir, texels, flags):
    src, dst = os.path.join(str(tmp_dir), "texels.bin"), os.path.join(str(tmp_dir), "blocks.bin")
    np.ascontiguousarray(texels, dtype=np.uint8).tofile(src)
    subprocess.run([exe, src, dst, str(flags)], check=True)
    return np.fromfile(dst, dtype=np.uint8).reshape(-1, 16)
