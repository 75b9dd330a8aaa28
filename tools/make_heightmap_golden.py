#!/usr/bin/env python3
"""Records tests/golden/heightmap_ref.npz and heightmap_ref_sha256.json: the outputs of the REFERENCE'S OWN _ComputeNMap (with its
_EvaluateColor and _EvaluateRow) on seeded RGBA32F and RGBA16F height maps, into RGBA32F (the unrounded normal) and RGBA16F targets.
Run by hand, never by build() or a test:

    python tools/make_heightmap_golden.py REFERENCE_ROOT [WORK_DIR]

Nothing of the reference is in this file.  At run time it cuts the three functions out of DirectXTexNormalMaps.cpp (found by their first
lines), writes them into WORK_DIR next to the harness below, and compiles the lot over oracle/ref_build/dxmath_stub with -ffp-contract=off.
The harness is glue: the component getters, XMVectorSetZ, XMVectorNegate, XMVectorMultiplyAdd as a multiply then an add (its SSE form),
XMVector3Cross as DirectXMath's six products and three differences, XMVector3Normalize in its SSE form (the squares summed (x + y) + z, a
square root, true divides, NaN for an infinite length), the four constants, _GetConvertFlags and the scanline load / store for
R32G32B32A32_FLOAT and R16G16B16A16_FLOAT in the reading tools/make_mipgen_golden.py states, and an allocator that fills with 0xCD.

Which NaN a divide gives is the machine's choice, so every NaN is recorded as 0x7FC00000 (0x7E00 in a half).  Cases: tests/_height_normal.py
golden_cases().  Small cases go into the npz whole (input and both outputs), large ones as SHA-256 of input and outputs.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _height_normal as H  # noqa: E402

HARNESS = r"""
#include <assert.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <vector>
#include <directxmath.h>

#define _In_
#define _In_reads_(n)
#define _Out_writes_(n)
typedef long HRESULT;
typedef unsigned long DWORD;
#define S_OK 0L
#define E_FAIL (-1L)
#define E_INVALIDARG (-2L)
#define E_OUTOFMEMORY (-3L)
#define E_POINTER (-4L)
#define ERROR_NOT_SUPPORTED 50L
#define HRESULT_FROM_WIN32(x) (-(long)(x) - 100L)
enum DXGI_FORMAT { DXGI_FORMAT_R32G32B32A32_FLOAT = 2, DXGI_FORMAT_R16G16B16A16_FLOAT = 10 };
enum CNMAP_FLAGS { CNMAP_CHANNEL_RED = 0x1, CNMAP_CHANNEL_GREEN = 0x2, CNMAP_CHANNEL_BLUE = 0x3, CNMAP_CHANNEL_ALPHA = 0x4, CNMAP_CHANNEL_LUMINANCE = 0x5,
                   CNMAP_MIRROR_U = 0x1000, CNMAP_MIRROR_V = 0x2000, CNMAP_INVERT_SIGN = 0x4000, CNMAP_COMPUTE_OCCLUSION = 0x8000 };
enum CONVERT_FLAGS { CONVF_FLOAT = 0x1, CONVF_UNORM = 0x2, CONVF_SNORM = 0x8 };
#define memcpy_s(dst, dstsize, src, n) memcpy((dst), (src), (n))

namespace DirectX {
/* glue: getters and lane arithmetic, each operation rounded to fp32 on its own */
inline float XMVectorGetY(FXMVECTOR v) { return v.f[1]; }
inline float XMVectorGetZ(FXMVECTOR v) { return v.f[2]; }
inline float XMVectorGetW(FXMVECTOR v) { return v.f[3]; }
inline XMVECTOR XMVectorSetZ(FXMVECTOR v, float z) { XMVECTOR r = v; r.f[2] = z; return r; }
inline XMVECTOR XMVectorNegate(FXMVECTOR v) { XMVECTOR r; for (int i = 0; i < 4; i++) r.f[i] = -v.f[i]; return r; }
/* XMVectorMultiplyAdd in its SSE form: _mm_mul_ps, then _mm_add_ps */
inline XMVECTOR XMVectorMultiplyAdd(FXMVECTOR a, FXMVECTOR b, FXMVECTOR c) { XMVECTOR r; for (int i = 0; i < 4; i++) { float p = a.f[i] * b.f[i]; r.f[i] = p + c.f[i]; } return r; }
/* six products, three differences */
inline XMVECTOR XMVector3Cross(FXMVECTOR a, FXMVECTOR b)
{
    XMVECTOR r;
    r.f[0] = (a.f[1] * b.f[2]) - (a.f[2] * b.f[1]);
    r.f[1] = (a.f[2] * b.f[0]) - (a.f[0] * b.f[2]);
    r.f[2] = (a.f[0] * b.f[1]) - (a.f[1] * b.f[0]);
    r.f[3] = 0.f;
    return r;
}
/* the SSE form: (x*x + y*y) + z*z, sqrtps, divps; a zero length gives zero, an infinite one NaN */
inline XMVECTOR XMVector3Normalize(FXMVECTOR v)
{
    const float sq = (v.f[0] * v.f[0] + v.f[1] * v.f[1]) + v.f[2] * v.f[2];
    const float m = sqrtf(sq);
    XMVECTOR r;
    for (int i = 0; i < 4; i++) r.f[i] = v.f[i] / m;
    if (m == 0.f) for (int i = 0; i < 4; i++) r.f[i] = 0.f;
    if (sq == INFINITY) for (int i = 0; i < 4; i++) r.u[i] = 0x7FC00000u;
    return r;
}
static const XMVECTORF32 g_XMNegIdentityR0 = {{{-1.f, 0.f, 0.f, 0.f}}};
static const XMVECTORF32 g_XMNegIdentityR1 = {{{0.f, -1.f, 0.f, 0.f}}};
static const XMVECTORF32 g_XMOneHalf = {{{0.5f, 0.5f, 0.5f, 0.5f}}};
static const XMVECTORF32 g_XMNegativeOneHalf = {{{-0.5f, -0.5f, -0.5f, -0.5f}}};

struct aligned_deleter { void operator()(void* p) { free(p); } };
typedef std::unique_ptr<XMVECTOR, aligned_deleter> ScopedAlignedArrayXMVECTOR;
typedef std::unique_ptr<float, aligned_deleter> ScopedAlignedArrayFloat;
inline void* _aligned_malloc(size_t n, size_t a) { void* p = nullptr; if (posix_memalign(&p, a, n ? n : a)) return nullptr; memset(p, 0xCD, n); return p; }

struct Image { size_t width, height; DXGI_FORMAT format; size_t rowPitch; uint8_t* pixels; };
static DWORD _GetConvertFlags(DXGI_FORMAT f) { return (f == DXGI_FORMAT_R32G32B32A32_FLOAT || f == DXGI_FORMAT_R16G16B16A16_FLOAT) ? CONVF_FLOAT : 0; }

/* IEEE binary16 <-> binary32 in integer arithmetic: the widening is exact, the narrowing rounds to nearest even */
static float half_to_float(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    uint32_t e = (h >> 10) & 31u, m = h & 0x3ffu, bits;
    if (e == 31u) bits = sign | 0x7f800000u | (m << 13);
    else if (e != 0u) bits = sign | ((e + 112u) << 23) | (m << 13);
    else if (m == 0u) bits = sign;
    else { e = 113u; while (!(m & 0x400u)) { m <<= 1; e--; } bits = sign | (e << 23) | ((m & 0x3ffu) << 13); }
    float f; memcpy(&f, &bits, 4); return f;
}
static uint16_t float_to_half(float f)
{
    uint32_t x; memcpy(&x, &f, 4);
    const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (x > 0x7f800000u ? 0x200u : 0u));
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);
    if (x < 0x33000001u) return sign;
    uint32_t m, shift;
    if (x < 0x38800000u) { m = (x & 0x7fffffu) | 0x800000u; shift = 126u - (x >> 23); }
    else { m = x - 0x38000000u; shift = 13u; }
    uint32_t r = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1u);
    if (rem > halfway || (rem == halfway && (r & 1u))) r++;
    return (uint16_t)(sign | r);
}

/* R32G32B32A32_FLOAT: the bytes as they are.  R16G16B16A16_FLOAT: widened on load; clamped to +-65504 and narrowed on store */
static bool _LoadScanline(XMVECTOR* dst, size_t count, const uint8_t* src, size_t size, DXGI_FORMAT format)
{
    if (format == DXGI_FORMAT_R32G32B32A32_FLOAT) { if (size < count * 16) return false; memcpy(dst, src, count * 16); return true; }
    if (size < count * 8) return false;
    const uint16_t* h = reinterpret_cast<const uint16_t*>(src);
    for (size_t i = 0; i < count; i++) for (int k = 0; k < 4; k++) dst[i].f[k] = half_to_float(h[4 * i + k]);
    return true;
}
static bool _StoreScanline(void* dst, size_t size, DXGI_FORMAT format, const XMVECTOR* src, size_t count)
{
    if (format == DXGI_FORMAT_R32G32B32A32_FLOAT) { if (size < count * 16) return false; memcpy(dst, src, count * 16); return true; }
    if (size < count * 8) return false;
    uint16_t* h = reinterpret_cast<uint16_t*>(dst);
    for (size_t i = 0; i < count; i++)
        for (int k = 0; k < 4; k++) {
            float v = src[i].f[k];
            v = (-65504.f > v) ? -65504.f : v;
            v = (65504.f < v) ? 65504.f : v;
            h[4 * i + k] = float_to_half(v);
        }
    return true;
}

#include "cut_normalmaps.inc"
} // namespace DirectX

using namespace DirectX;

/* heightmap_ref SRCFORMAT DSTFORMAT W H FLAGS(hex) AMPLITUDE(hex bits of a float) in.bin out.bin */
int main(int argc, char** argv)
{
    if (argc != 9) return 2;
    const DXGI_FORMAT sf = (DXGI_FORMAT)atoi(argv[1]), df = (DXGI_FORMAT)atoi(argv[2]);
    const size_t w = strtoul(argv[3], 0, 10), h = strtoul(argv[4], 0, 10);
    const DWORD flags = (DWORD)strtoul(argv[5], 0, 16);
    const uint32_t abits = (uint32_t)strtoul(argv[6], 0, 16);
    float amplitude; memcpy(&amplitude, &abits, 4);
    const size_t spx = sf == DXGI_FORMAT_R32G32B32A32_FLOAT ? 16 : 8, dpx = df == DXGI_FORMAT_R32G32B32A32_FLOAT ? 16 : 8;
    std::vector<uint8_t> in(w * h * spx), out(w * h * dpx, 0xEE);
    FILE* f = fopen(argv[7], "rb");
    if (!f || fread(in.data(), 1, in.size(), f) != in.size()) return 3;
    fclose(f);
    const Image src{w, h, sf, w * spx, in.data()}, dst{w, h, df, w * dpx, out.data()};
    if (_ComputeNMap(src, flags, amplitude, df, dst) != S_OK) return 4;
    f = fopen(argv[8], "wb");
    fwrite(out.data(), 1, out.size(), f);
    fclose(f);
    return 0;
}
"""


def cut(lines, first_marker, end_marker):
    """The lines from the one that contains first_marker up to, not including, the next one that contains end_marker."""
    i0 = next(i for i, l in enumerate(lines) if first_marker in l)
    i1 = next(i for i in range(i0 + 1, len(lines)) if end_marker in lines[i])
    return lines[i0:i1]


def build(ref_root, work):
    path = os.path.join(ref_root, "3rdParty", "DirectXTex", "DirectXTex", "DirectXTexNormalMaps.cpp")
    with open(path, encoding="latin-1") as f:
        lines = f.readlines()
    text = cut(lines, "static inline float _EvaluateColor(", "static void _EvaluateRow(") \
        + cut(lines, "static void _EvaluateRow(", "static HRESULT _ComputeNMap(") \
        + cut(lines, "static HRESULT _ComputeNMap(", "// Entry points")
    with open(os.path.join(work, "cut_normalmaps.inc"), "w") as f:
        f.writelines(text)
    with open(os.path.join(work, "harness.cpp"), "w") as f:
        f.write(HARNESS)
    exe = os.path.join(work, "heightmap_ref")
    subprocess.run(["g++", "-std=c++17", "-O1", "-w", "-ffp-contract=off", "-I", os.path.join(ROOT, "oracle", "ref_build", "dxmath_stub"), "-I", work,
                    os.path.join(work, "harness.cpp"), "-o", exe], check=True)
    return exe


FORMAT = {"float": 2, "half": 10}


def run(exe, work, base, src, dst, ops):
    h, w = base.shape[:2]
    a, b = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
    base.tofile(a)
    flags = ((ops >> 8) & 15) | (ops & 0xF000)                    # the channel in the low bits, the mirror / invert / occlusion bits where they are
    amp = int(np.array(H.amplitude_of(ops), dtype=np.float32).view(np.uint32))
    subprocess.run([exe, str(FORMAT[src]), str(FORMAT[dst]), str(w), str(h), f"{flags:x}", f"{amp:x}", a, b], check=True)
    if dst == "float":
        return H.canonical_nan(np.fromfile(b, dtype=np.float32).reshape(h, w, 4))
    out = np.fromfile(b, dtype=np.uint16).reshape(h, w, 4)
    out[(out & 0x7FFF) > 0x7C00] = 0x7E00
    return out


def main():
    ref_root = sys.argv[1]
    work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="heightmap_ref_")
    os.makedirs(work, exist_ok=True)
    exe = build(ref_root, work)
    arrays, pins = {}, {}
    for c in H.golden_cases():
        w, h = c["width"], c["height"]
        base = H.golden_input(c["src"], c["content"], h, w, c["seed"])
        name = H.golden_name(c)
        f32 = run(exe, work, base, c["src"], "float", c["ops"])
        f16 = run(exe, work, base, c["src"], "half", c["ops"])
        stored = w * h <= H.GOLDEN_STORED
        if stored:
            arrays[name + "_in"], arrays[name + "_f32"], arrays[name + "_f16"] = base, f32, f16
        first = 1 if H.golden_skips_row0(c) else 0                # the stated divergence: the hashes of such a case leave row 0 out
        pins[name] = {"stored": stored, "first_row": first, "input_sha256": hashlib.sha256(base.tobytes()).hexdigest(),
                      "f32_sha256": hashlib.sha256(f32[first:].tobytes()).hexdigest(), "f16_sha256": hashlib.sha256(f16[first:].tobytes()).hexdigest()}
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(H.GOLDEN, **arrays)
    with open(H.GOLDEN_SHA, "w") as f:
        json.dump(pins, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(pins), "cases ->", gold, os.path.getsize(H.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
