#!/usr/bin/env python3
"""Records tests/golden/mipgen_ref.npz and mipgen_ref_sha256.json: the outputs of the REFERENCE'S OWN _Generate2DMipsBoxFilter,
_Generate2DMipsLinearFilter and _CreateLinearFilter on seeded RGBA16F images.  Run by hand, never by build() or a test:

    python tools/make_mipgen_golden.py REFERENCE_ROOT [WORK_DIR]

Nothing of the reference is in this file.  At run time it cuts the box-filter helpers and the linear-filter helpers out of Filters.h and
the two function bodies out of DirectXTexMipmaps.cpp (found by their first lines), writes them into WORK_DIR next to the harness below, and
compiles the lot over oracle/ref_build/dxmath_stub with -ffp-contract=off.  The harness is glue: a ScratchImage of plain arrays, the vector
operators the cut text uses, and the two scanline functions for R16G16B16A16_FLOAT, which are THIS FILE'S READING of
DirectXTexConvert.cpp:765-766 (XMLoadHalf4: the half widened exactly) and :1634-1646 (XMVectorClamp to +-65504, then XMStoreHalf4: round to
nearest even) -- the pin covers the filters, and the store only as far as that reading goes.

Cases: square and tall power-of-two sizes through the box filter, sizes that are no powers of two of every aspect through the linear one.
Wide power-of-two chains are left out: there the reference's box filter reads a stale scanline (include/itw_dispatch.h, "Stated
divergence").  Small cases go into the npz whole (input and every level), large ones as SHA-256 of input and of the concatenated levels.
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

# (width, height, seed)
BOX_CASES = [(2, 2, 1), (4, 4, 2), (8, 8, 3), (1, 8, 4), (2, 16, 5), (16, 16, 6), (8, 32, 7), (64, 64, 8), (128, 128, 9), (64, 256, 10), (1, 2, 11)]
LINEAR_CASES = [(3, 1, 21), (1, 3, 22), (5, 3, 23), (7, 7, 24), (3, 5, 25), (12, 20, 26), (100, 36, 27), (127, 339, 28), (96, 64, 29), (6, 1, 30), (1, 6, 31)]
FILTER_PAIRS = [(1, 1), (2, 1), (3, 1), (5, 2), (7, 3), (12, 6), (36, 18), (96, 48), (100, 50), (127, 63), (339, 169), (4000, 2000), (3000, 1500), (8191, 4095)]
SMALL = 1024          # texels of the base up to which a case is stored whole

HARNESS = r"""
#include <assert.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <new>
#include <utility>
#include <vector>
#include <directxmath.h>

#define XMGLOBALCONST static const
#define _In_
#define _Out_writes_(n)
typedef long HRESULT;
typedef unsigned long DWORD;
#define S_OK 0L
#define E_FAIL (-1L)
#define E_INVALIDARG (-2L)
#define E_OUTOFMEMORY (-3L)
#define E_POINTER (-4L)
enum DXGI_FORMAT { DXGI_FORMAT_R16G16B16A16_FLOAT = 10 };
enum { TEX_FILTER_WRAP_U = 0x1, TEX_FILTER_WRAP_V = 0x2 };

namespace DirectX {
/* glue: lane arithmetic, each operation rounded to fp32 on its own */
inline XMVECTOR XMVectorAdd(FXMVECTOR a, FXMVECTOR b) { XMVECTOR r; for (int i = 0; i < 4; i++) r.f[i] = a.f[i] + b.f[i]; return r; }
inline XMVECTOR operator*(FXMVECTOR a, float s) { XMVECTOR r; for (int i = 0; i < 4; i++) r.f[i] = a.f[i] * s; return r; }
inline XMVECTOR operator*(float s, FXMVECTOR a) { XMVECTOR r; for (int i = 0; i < 4; i++) r.f[i] = a.f[i] * s; return r; }
inline XMVECTOR operator+(FXMVECTOR a, FXMVECTOR b) { return XMVectorAdd(a, b); }
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
inline void* _aligned_malloc(size_t n, size_t a) { void* p = nullptr; if (posix_memalign(&p, a, n ? n : a)) return nullptr; memset(p, 0, n); return p; }
inline bool ispow2(size_t x) { return x != 0 && (x & (x - 1)) == 0; }

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

/* this file's reading of DirectXTexConvert.cpp:765-766 and :1634-1646 for R16G16B16A16_FLOAT */
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

/* mipgen_ref box|linear W H in.bin out.bin   or   mipgen_ref filter SOURCE DEST out.bin */
int main(int argc, char** argv)
{
    if (argc == 5 && !strcmp(argv[1], "filter")) {
        const size_t source = strtoul(argv[2], 0, 10), dest = strtoul(argv[3], 0, 10);
        std::vector<LinearFilter> lf(dest);
        _CreateLinearFilter(source, dest, false, lf.data());
        FILE* f = fopen(argv[4], "wb");
        for (size_t i = 0; i < dest; i++) {
            const int64_t u[2] = {(int64_t)lf[i].u0, (int64_t)lf[i].u1};
            const float w[2] = {lf[i].weight0, lf[i].weight1};
            fwrite(u, 8, 2, f); fwrite(w, 4, 2, f);
        }
        fclose(f);
        return 0;
    }
    if (argc != 6) return 2;
    const bool box = !strcmp(argv[1], "box");
    const size_t w = strtoul(argv[2], 0, 10), h = strtoul(argv[3], 0, 10);
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
    FILE* f = fopen(argv[4], "rb");
    if (!f || fread(store[0].data(), 1, store[0].size(), f) != store[0].size()) return 3;
    fclose(f);
    if (levels > 1) {
        const HRESULT hr = box ? _Generate2DMipsBoxFilter(levels, 0, chain, 0) : _Generate2DMipsLinearFilter(levels, 0, chain, 0);
        if (hr != S_OK) return 4;
    }
    f = fopen(argv[5], "wb");
    for (size_t l = 1; l < levels; l++) fwrite(store[l].data(), 1, store[l].size(), f);
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
    dxtex = os.path.join(ref_root, "3rdParty", "DirectXTex", "DirectXTex")
    with open(os.path.join(dxtex, "Filters.h"), encoding="latin-1") as f:
        fl = f.readlines()
    with open(os.path.join(dxtex, "DirectXTexMipmaps.cpp"), encoding="latin-1") as f:
        ml = f.readlines()
    filters = cut(fl, "g_boxScale =", "#define AVERAGE8") + cut(fl, "struct LinearFilter", "#define TRILINEAR_INTERPOLATE")
    mipmaps = cut(ml, "static HRESULT _Generate2DMipsBoxFilter(", "//--- 2D Linear Filter ---") \
        + cut(ml, "static HRESULT _Generate2DMipsLinearFilter(", "//--- 2D Cubic Filter ---")
    with open(os.path.join(work, "cut_filters.inc"), "w") as f:
        f.writelines(filters)
    with open(os.path.join(work, "cut_mipmaps.inc"), "w") as f:
        f.writelines(mipmaps)
    with open(os.path.join(work, "harness.cpp"), "w") as f:
        f.write(HARNESS)
    exe = os.path.join(work, "mipgen_ref")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "oracle", "ref_build", "dxmath_stub"), "-I", work,
                    os.path.join(work, "harness.cpp"), "-o", exe], check=True)
    return exe


def run_chain(exe, work, kind, base):
    h, w = base.shape[:2]
    src, dst = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
    base.tofile(src)
    subprocess.run([exe, kind, str(w), str(h), src, dst], check=True)
    flat = np.fromfile(dst, dtype=np.uint16)
    out, at = [], 0
    for l in range(1, M.levels_of(w, h)):
        lw, lh = M.level_size(w, h, l)
        out.append(flat[at:at + lw * lh * 4].reshape(lh, lw, 4))
        at += lw * lh * 4
    assert at == flat.size
    return out


def main():
    ref_root = sys.argv[1]
    work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="mipgen_ref_")
    os.makedirs(work, exist_ok=True)
    exe = build(ref_root, work)
    arrays, pins = {}, {"cases": {}}
    for kind, cases in (("box", BOX_CASES), ("linear", LINEAR_CASES)):
        for w, h, seed in cases:
            base = M.seeded_half_image(h, w, seed)
            levels = run_chain(exe, work, kind, base)
            name = f"{kind}_{w}x{h}"
            entry = {"filter": kind, "width": w, "height": h, "seed": seed, "stored": w * h <= SMALL,
                     "input_sha256": hashlib.sha256(base.tobytes()).hexdigest(),
                     "levels_sha256": hashlib.sha256(b"".join(np.ascontiguousarray(l).tobytes() for l in levels)).hexdigest()}
            if entry["stored"]:
                arrays[name + "_in"] = base
                for i, l in enumerate(levels):
                    arrays[f"{name}_l{i + 1}"] = l
            pins["cases"][name] = entry
    for source, dest in FILTER_PAIRS:
        dst = os.path.join(work, "filter.bin")
        subprocess.run([exe, "filter", str(source), str(dest), dst], check=True)
        rec = np.fromfile(dst, dtype=np.dtype([("u0", "<i8"), ("u1", "<i8"), ("w0", "<f4"), ("w1", "<f4")]))
        arrays[f"filter_{source}_{dest}"] = np.stack([rec["u0"].astype(np.float64), rec["w0"].astype(np.float64),
                                                      rec["u1"].astype(np.float64), rec["w1"].astype(np.float64)])
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "mipgen_ref.npz"), **arrays)
    with open(os.path.join(gold, "mipgen_ref_sha256.json"), "w") as f:
        json.dump(pins, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(pins["cases"]), "cases,", len(FILTER_PAIRS), "filter tables ->", gold)


if __name__ == "__main__":
    main()
