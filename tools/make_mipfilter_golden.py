#!/usr/bin/env python3
"""Records tests/golden/mipfilter_ref.npz and mipfilter_ref_sha256.json: the outputs of the REFERENCE'S OWN _Generate2DMipsCubicFilter,
_Generate2DMipsTriangleFilter, _CreateCubicFilter and TriangleFilter::_Create on seeded RGBA16F images, under clamp and wrap addressing.
Run by hand, never by build() or a test:

    python tools/make_mipfilter_golden.py REFERENCE_ROOT [WORK_DIR]

Nothing of the reference is in this file.  At run time it cuts the cubic helpers (the constants, bounduvw, CubicFilter, _CreateCubicFilter,
CUBIC_INTERPOLATE) and the TriangleFilter namespace out of Filters.h and the two function bodies out of DirectXTexMipmaps.cpp (found by
their first lines), writes them into WORK_DIR next to the harness below, and compiles the lot over oracle/ref_build/dxmath_stub with
-ffp-contract=off.  The harness is glue: a ScratchImage of plain arrays, the vector operators the cut text uses, XMVectorReplicate,
XMVectorMultiplyAdd as a multiply then an add (its SSE form), and the two scanline functions for R16G16B16A16_FLOAT in the reading
tools/make_mipgen_golden.py states.

Cases: every size under both filters and under clamp, wrap U, wrap V and wrap UV.  Small cases go into the npz whole (input and every
level), large ones as SHA-256 of input and of the concatenated levels.  The per-axis tables likewise: whole up to 339 source texels, as
SHA-256 of their bytes above.
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
import _mipgen as M  # noqa: E402
import _mip_filters as MF  # noqa: E402

# (width, height, seed)
CASES = [(2, 2, 41), (1, 8, 42), (8, 1, 43), (4, 4, 44), (3, 5, 45), (5, 3, 46), (7, 7, 47), (12, 20, 48), (16, 16, 49), (64, 64, 50), (256, 4, 51),
         (4, 256, 52), (96, 64, 53), (100, 36, 54), (127, 339, 55)]
FILTER_PAIRS = [(1, 1), (2, 1), (3, 1), (5, 2), (7, 3), (12, 6), (127, 63), (339, 169), (4000, 2000), (3000, 1500), (8191, 4095)]
SMALL = 1024          # texels of the base up to which a case is stored whole
SMALL_TABLE = 339     # source texels up to which a table is stored whole

HARNESS = r"""
#include <assert.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <new>
#include <utility>
#include <vector>
#include <directxmath.h>

#define XMGLOBALCONST static const
#define _In_
#define _Inout_
#define _Out_writes_(n)
typedef long HRESULT;
typedef unsigned long DWORD;
#define S_OK 0L
#define E_FAIL (-1L)
#define E_INVALIDARG (-2L)
#define E_OUTOFMEMORY (-3L)
#define E_POINTER (-4L)
#define FAILED(hr) ((hr) < 0)
enum DXGI_FORMAT { DXGI_FORMAT_R16G16B16A16_FLOAT = 10, DXGI_FORMAT_R10G10B10A2_UNORM = 24, DXGI_FORMAT_R10G10B10A2_UINT = 25 };
enum { TEX_FILTER_WRAP_U = 0x1, TEX_FILTER_WRAP_V = 0x2, TEX_FILTER_MIRROR_U = 0x10, TEX_FILTER_MIRROR_V = 0x20 };

namespace DirectX {
/* glue: lane arithmetic, each operation rounded to fp32 on its own */
inline XMVECTOR XMVectorAdd(FXMVECTOR a, FXMVECTOR b) { XMVECTOR r; for (int i = 0; i < 4; i++) r.f[i] = a.f[i] + b.f[i]; return r; }
inline XMVECTOR operator+(FXMVECTOR a, FXMVECTOR b) { return XMVectorAdd(a, b); }
inline XMVECTOR operator-(FXMVECTOR a, FXMVECTOR b) { return XMVectorSubtract(a, b); }
inline XMVECTOR operator*(FXMVECTOR a, FXMVECTOR b) { return XMVectorMultiply(a, b); }
inline XMVECTOR XMVectorReplicate(float v) { return XMVectorSet(v, v, v, v); }
/* XMVectorMultiplyAdd in its SSE form: _mm_mul_ps, then _mm_add_ps */
inline XMVECTOR XMVectorMultiplyAdd(FXMVECTOR a, FXMVECTOR b, FXMVECTOR c) { return XMVectorAdd(XMVectorMultiply(a, b), c); }
static const XMVECTORF32 g_HalfMin = {{{-65504.f, -65504.f, -65504.f, -65504.f}}};
static const XMVECTORF32 g_HalfMax = {{{65504.f, 65504.f, 65504.f, 65504.f}}};
inline XMVECTOR XMVectorClamp(FXMVECTOR v, FXMVECTOR lo, FXMVECTOR hi)
{
    XMVECTOR r;
    for (int i = 0; i < 4; i++) { float t = (lo.f[i] > v.f[i]) ? lo.f[i] : v.f[i]; r.f[i] = (hi.f[i] < t) ? hi.f[i] : t; }
    return r;
}

struct aligned_deleter { void operator()(void* p) { free(p); } };
typedef std::unique_ptr<XMVECTOR, aligned_deleter> ScopedAlignedArrayXMVECTOR;
inline void* _aligned_malloc(size_t n, size_t a) { void* p = nullptr; if (posix_memalign(&p, a, n ? n : a)) return nullptr; memset(p, 0xCD, n); return p; }

struct Image { size_t width, height; DXGI_FORMAT format; size_t rowPitch; uint8_t* pixels; };
struct TexMetadata { size_t width, height; };
struct ScratchImage {
    TexMetadata meta; std::vector<Image> images; size_t levels;
    const Image* GetImages() const { return images.data(); }
    const TexMetadata& GetMetadata() const { return meta; }
    const Image* GetImage(size_t level, size_t item, size_t) const { return &images[item * levels + level]; }
};

/* IEEE binary16 <-> binary32 in integer arithmetic: the widening is exact, the narrowing rounds to nearest even (denormals, overflow to inf) */
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
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                 /* rounds to 65536 or above */
    if (x < 0x33000001u) return sign;                                       /* at most half of the smallest denormal */
    uint32_t m, shift;
    if (x < 0x38800000u) { m = (x & 0x7fffffu) | 0x800000u; shift = 126u - (x >> 23); }   /* denormal result */
    else { m = x - 0x38000000u; shift = 13u; }
    uint32_t r = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1u);
    if (rem > halfway || (rem == halfway && (r & 1u))) r++;
    return (uint16_t)(sign | r);
}

/* the reading of DirectXTexConvert.cpp:765-766 and :1634-1646 for R16G16B16A16_FLOAT that tools/make_mipgen_golden.py states */
static bool _LoadScanlineLinear(XMVECTOR* dst, size_t count, const uint8_t* src, size_t size, DXGI_FORMAT, DWORD)
{
    if (size < count * 8) return false;
    const uint16_t* h = reinterpret_cast<const uint16_t*>(src);
    for (size_t i = 0; i < count; i++) for (int k = 0; k < 4; k++) dst[i].f[k] = half_to_float(h[4 * i + k]);
    return true;
}
static bool _StoreScanlineLinear(void* dst, size_t size, DXGI_FORMAT, XMVECTOR* src, size_t count, DWORD)
{
    if (size < count * 8) return false;
    uint16_t* h = reinterpret_cast<uint16_t*>(dst);
    for (size_t i = 0; i < count; i++) {
        XMVECTOR v = XMVectorClamp(src[i], g_HalfMin, g_HalfMax);
        for (int k = 0; k < 4; k++) h[4 * i + k] = float_to_half(v.f[k]);
    }
    return true;
}

#include "cut_filters.inc"
#include "cut_mipmaps.inc"
} // namespace DirectX

using namespace DirectX;

/* mipfilter_ref cubic|triangle WRAPBITS W H in.bin out.bin   or   mipfilter_ref cubictable|triangletable WRAP SOURCE DEST out.bin */
int main(int argc, char** argv)
{
    if (argc == 6 && !strcmp(argv[1], "cubictable")) {
        const bool wrap = atoi(argv[2]) != 0;
        const size_t source = strtoul(argv[3], 0, 10), dest = strtoul(argv[4], 0, 10);
        std::vector<CubicFilter> cf(dest);
        _CreateCubicFilter(source, dest, wrap, false, cf.data());
        FILE* f = fopen(argv[5], "wb");
        for (size_t i = 0; i < dest; i++) {
            const int32_t u[4] = {(int32_t)cf[i].u0, (int32_t)cf[i].u1, (int32_t)cf[i].u2, (int32_t)cf[i].u3};
            fwrite(u, 4, 4, f); fwrite(&cf[i].x, 4, 1, f);
        }
        fclose(f);
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "triangletable")) {
        const bool wrap = atoi(argv[2]) != 0;
        const size_t source = strtoul(argv[3], 0, 10), dest = strtoul(argv[4], 0, 10);
        std::unique_ptr<TriangleFilter::Filter> tf;
        if (TriangleFilter::_Create(source, dest, wrap, tf) != S_OK) return 5;
        FILE* f = fopen(argv[5], "wb");
        const uint8_t* p = reinterpret_cast<const uint8_t*>(tf->from);
        const uint8_t* end = reinterpret_cast<const uint8_t*>(tf.get()) + tf->sizeInBytes;
        for (size_t u = 0; p < end; u++) {
            const TriangleFilter::FilterFrom* from = reinterpret_cast<const TriangleFilter::FilterFrom*>(p);
            for (size_t j = 0; j < from->count; j++) {
                const int32_t idx[2] = {(int32_t)u, (int32_t)from->to[j].u};
                fwrite(idx, 4, 2, f); fwrite(&from->to[j].weight, 4, 1, f);
            }
            p += from->sizeInBytes;
        }
        fclose(f);
        return 0;
    }
    if (argc != 7) return 2;
    const bool cubic = !strcmp(argv[1], "cubic");
    const DWORD filter = (DWORD)atoi(argv[2]);
    const size_t w = strtoul(argv[3], 0, 10), h = strtoul(argv[4], 0, 10);
    size_t levels = 1;
    for (size_t m = w > h ? w : h; m > 1; m >>= 1) levels++;
    ScratchImage chain;
    chain.meta.width = w; chain.meta.height = h; chain.levels = levels;
    std::vector<std::vector<uint8_t>> store(levels);
    for (size_t l = 0; l < levels; l++) {
        const size_t lw = (w >> l) ? (w >> l) : 1, lh = (h >> l) ? (h >> l) : 1;
        store[l].assign(lw * lh * 8, 0xEE);
        chain.images.push_back(Image{lw, lh, DXGI_FORMAT_R16G16B16A16_FLOAT, lw * 8, store[l].data()});
    }
    FILE* f = fopen(argv[5], "rb");
    if (!f || fread(store[0].data(), 1, store[0].size(), f) != store[0].size()) return 3;
    fclose(f);
    if (levels > 1) {
        const HRESULT hr = cubic ? _Generate2DMipsCubicFilter(levels, filter, chain, 0) : _Generate2DMipsTriangleFilter(levels, filter, chain, 0);
        if (hr != S_OK) return 4;
    }
    f = fopen(argv[6], "wb");
    for (size_t l = 1; l < levels; l++) fwrite(store[l].data(), 1, store[l].size(), f);
    fclose(f);
    return 0;
}
"""

CUBIC_TABLE = np.dtype([("u", "<i4", 4), ("x", "<f4")])
TRIANGLE_TABLE = np.dtype([("idx", "<i4", 2), ("w", "<f4")])


def cut(lines, first_marker, end_marker):
    """The lines from the one that contains first_marker up to, not including, the next one that contains end_marker."""
    i0 = next(i for i, l in enumerate(lines) if first_marker in l)
    i1 = next(i for i in range(i0 + 1, len(lines)) if end_marker in lines[i])
    return lines[i0:i1]


def build(ref_root, work):
    dxtex = os.path.join(ref_root, "3rdParty", "DirectXTex", "DirectXTex")
    with open(os.path.join(dxtex, "Filters.h"), encoding="latin-1") as f:
        fl = f.readlines()
    with open(os.path.join(dxtex, "DirectXTexMipmaps.cpp"), encoding="latin-1") as f:
        ml = f.readlines()
    # the cubic helpers, then the TriangleFilter namespace up to the line that closes it (which the second cut leaves out)
    filters = cut(fl, "g_cubicThird =", "// Triangle filtering helpers") + cut(fl, "namespace TriangleFilter", "}; // namespace") + ["}\n"]
    mipmaps = cut(ml, "static HRESULT _Generate2DMipsCubicFilter(", "//--- 2D Triangle Filter ---") \
        + cut(ml, "static HRESULT _Generate2DMipsTriangleFilter(", "// Generate volume mip-map helpers")
    with open(os.path.join(work, "cut_filters.inc"), "w") as f:
        f.writelines(filters)
    with open(os.path.join(work, "cut_mipmaps.inc"), "w") as f:
        f.writelines(mipmaps)
    with open(os.path.join(work, "harness.cpp"), "w") as f:
        f.write(HARNESS)
    exe = os.path.join(work, "mipfilter_ref")
    subprocess.run(["g++", "-std=c++17", "-O1", "-w", "-ffp-contract=off", "-I", os.path.join(ROOT, "oracle", "ref_build", "dxmath_stub"), "-I", work,
                    os.path.join(work, "harness.cpp"), "-o", exe], check=True)
    return exe


def run_chain(exe, work, kind, wrap, base):
    h, w = base.shape[:2]
    src, dst = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
    base.tofile(src)
    subprocess.run([exe, kind, str((1 if "u" in wrap else 0) | (2 if "v" in wrap else 0)), str(w), str(h), src, dst], check=True)
    flat = np.fromfile(dst, dtype=np.uint16)
    out, at = [], 0
    for l in range(1, M.levels_of(w, h)):
        lw, lh = M.level_size(w, h, l)
        out.append(flat[at:at + lw * lh * 4].reshape(lh, lw, 4))
        at += lw * lh * 4
    assert at == flat.size
    return out


def case_name(kind, wrap, w, h):
    return f"{kind}_{wrap or 'clamp'}_{w}x{h}"


def table_name(kind, wrap, source, dest):
    return f"{kind}table_{'wrap' if wrap else 'clamp'}_{source}_{dest}"


def main():
    ref_root = sys.argv[1]
    work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="mipfilter_ref_")
    os.makedirs(work, exist_ok=True)
    exe = build(ref_root, work)
    arrays, pins = {}, {"cases": {}, "tables": {}}
    for w, h, seed in CASES:
        base = MF.seeded_half_image(h, w, seed)
        if w * h <= SMALL:
            arrays[f"in_{w}x{h}"] = base
        for kind in ("cubic", "triangle"):
            for wrap in MF.WRAPS:
                levels = run_chain(exe, work, kind, wrap, base)
                name = case_name(kind, wrap, w, h)
                entry = {"filter": kind, "wrap": wrap, "width": w, "height": h, "seed": seed, "stored": w * h <= SMALL,
                         "input_sha256": hashlib.sha256(base.tobytes()).hexdigest(),
                         "levels_sha256": hashlib.sha256(b"".join(np.ascontiguousarray(l).tobytes() for l in levels)).hexdigest()}
                if entry["stored"]:
                    for i, l in enumerate(levels):
                        arrays[f"{name}_l{i + 1}"] = l
                pins["cases"][name] = entry
    for source, dest in FILTER_PAIRS:
        for kind, dtype in (("cubic", CUBIC_TABLE), ("triangle", TRIANGLE_TABLE)):
            for wrap in (0, 1):
                dst = os.path.join(work, "table.bin")
                subprocess.run([exe, kind + "table", str(wrap), str(source), str(dest), dst], check=True)
                rec = np.fromfile(dst, dtype=dtype)
                name = table_name(kind, wrap, source, dest)
                pins["tables"][name] = {"entries": int(rec.size), "sha256": hashlib.sha256(rec.tobytes()).hexdigest(), "stored": source <= SMALL_TABLE}
                if source <= SMALL_TABLE:
                    arrays[name + "_i"] = rec["u" if kind == "cubic" else "idx"].copy()
                    arrays[name + "_w"] = rec["x" if kind == "cubic" else "w"].copy()
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "mipfilter_ref.npz"), **arrays)
    with open(os.path.join(gold, "mipfilter_ref_sha256.json"), "w") as f:
        json.dump(pins, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(pins["cases"]), "cases,", len(pins["tables"]), "tables ->", gold)


if __name__ == "__main__":
    main()
