// mip_filters.hpp -- the arithmetic of the two further mip filters (include/itw_dispatch.h, "Mip chains: cubic and triangle"): DirectXTex's
// non-WIC 2D cubic filter (DirectXTexMipmaps.cpp:921-1103; _CreateCubicFilter, bounduvw and CUBIC_INTERPOLATE, Filters.h:123-205) and its
// triangle filter (:1107-1313; TriangleFilter::_Create, Filters.h:249-418).  IEEE fp32, one rounding per operation, on the host and in the
// kernels (the library is built with -ffp-contract=off).  The cubic taps are a few operations per lane and are formed in the kernel; the
// triangle filter's per-axis lists are built on the host, inverted, and travel to the device beside the chain's image table.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "mipgen.hpp"

namespace itw {

// which filter a chain takes: the default's choice between box and linear, or one filter on every level
// (point and linear by name are the free-size chain's, ITW_MIP_RESIZE; box is what its default resolves to at exactly 2:1)
enum MipFilterKind { MIP_FILTER_DEFAULT = 0, MIP_FILTER_CUBIC = 1, MIP_FILTER_TRIANGLE = 2, MIP_FILTER_POINT = 3, MIP_FILTER_LINEAR = 4, MIP_FILTER_BOX = 5 };

// bounduvw with mirror off: wrap folds one period, then the clamp (which alone remains for degenerate sources)
__host__ __device__ __forceinline__ int32_t mip_bound(int32_t u, int32_t maxu, bool wrap)
{
    if (wrap) {
        if (u < 0) u = maxu + u + 1;
        else if (u > maxu) u = u - maxu - 1;
    }
    u = u < maxu ? u : maxu;
    return u > 0 ? u : 0;
}

// one axis of _CreateCubicFilter: `scale` = float(source) / float(dest); b is the bounded isrcB, the taps are bound(b - 1 .. b + 2) and
// x = srcB - float(b)
struct MipCubicTap { int32_t b; float x; };
__host__ __device__ __forceinline__ MipCubicTap mip_cubic_tap(int32_t u, float scale, int32_t source, bool wrap)
{
    const float srcB = ((float)u + 0.5f) * scale - 0.5f;
    MipCubicTap t;
    t.b = mip_bound((int32_t)srcB, source - 1, wrap);
    t.x = srcB - (float)t.b;
    return t;
}

// ---- the free-size chain (ITW_MIP_RESIZE; resize.hip): the same per-axis arithmetic at any (source, dest) pair ------------------------------

// how one axis is addressed past its ends: bounduvw's three cases, wrap before mirror
enum MipAddress : uint32_t { MIP_ADDR_CLAMP = 0, MIP_ADDR_WRAP = 1, MIP_ADDR_MIRROR = 2 };

// bounduvw as written (Filters.h:123-153): wrap folds one period, mirror reflects about the edge, then the clamp
__host__ __device__ __forceinline__ int32_t mip_bound_addr(int32_t u, int32_t maxu, uint32_t addr)
{
    if (addr == MIP_ADDR_WRAP) {
        if (u < 0) u = maxu + u + 1;
        else if (u > maxu) u = u - maxu - 1;
    } else if (addr == MIP_ADDR_MIRROR) {
        if (u < 0) u = (-u) - 1;
        else if (u > maxu) u = maxu - (u - maxu - 1);
    }
    u = u < maxu ? u : maxu;
    return u > 0 ? u : 0;
}

// one axis of _CreateCubicFilter under any addressing; (int32_t)srcB truncates toward zero, so an upscale's first texels have x < 0
__host__ __device__ __forceinline__ MipCubicTap mip_cubic_tap_addr(int32_t u, float scale, int32_t source, uint32_t addr)
{
    const float srcB = ((float)u + 0.5f) * scale - 0.5f;
    MipCubicTap t;
    t.b = mip_bound_addr((int32_t)srcB, source - 1, addr);
    t.x = srcB - (float)t.b;
    return t;
}

// one axis of _CreateLinearFilter as written (Filters.h:66-102), its wrap branches included: weight0 is formed from isrcB AFTER the fold.
// The two last lines change nothing the reference computes: they keep a read inside the row where fp32 no longer holds the coordinate.
__host__ __device__ __forceinline__ MipTap mip_linear_tap_wrap(int32_t u, float scale, int32_t source, bool wrap)
{
    const float srcB = ((float)u + 0.5f) * scale + 0.5f;
    int32_t b = (int32_t)srcB;
    int32_t a = b - 1;
    if (a < 0) a = wrap ? source - 1 : 0;
    if (b >= source) b = wrap ? 0 : source - 1;
    if (a >= source) a = source - 1;
    if (b < 0) b = 0;
    MipTap t;
    t.u0 = a; t.u1 = b;
    t.w0 = 1.0f + (float)b - srcB;
    t.w1 = 1.0f - t.w0;
    return t;
}

// _ResizePointFilter's step along one axis, (source << 16) / dest in 64 bits, and the source index of destination u: the reference's
// running sum sx += inc is the product u * inc, and (u * inc) >> 16 < source for every u < dest
__host__ __device__ __forceinline__ uint64_t mip_point_step(int32_t source, int32_t dest) { return ((uint64_t)source << 16) / (uint64_t)dest; }
__host__ __device__ __forceinline__ int32_t mip_point_index(int32_t u, uint64_t step, int32_t source)
{
    const int32_t s = (int32_t)(((uint64_t)u * step) >> 16);
    return s < source ? s : source - 1;
}

// CUBIC_INTERPOLATE on one channel, in C++ operator order
__host__ __device__ __forceinline__ float mip_cubic_value(float p0, float p1, float p2, float p3, float x)
{
    const float third = 1.f / 3.f, sixth = 1.f / 6.f, half = 0.5f;
    const float a0 = p1;
    const float d0 = p0 - a0;
    const float d2 = p2 - a0;
    const float d3 = p3 - a0;
    float a1 = third * d0;
    a1 = d2 - a1;
    a1 = a1 - sixth * d3;
    const float a2 = half * d0 + half * d2;
    float a3 = sixth * d3 - sixth * d0;
    a3 = a3 - half * d2;
    const float x2 = x * x;
    const float x3 = x2 * x;
    float r = a0 + a1 * x;
    r = r + a2 * x2;
    return r + a3 * x3;
}

__device__ __forceinline__ MipTexel mip_cubic(const MipTexel& p0, const MipTexel& p1, const MipTexel& p2, const MipTexel& p3, float x)
{
    MipTexel r;
#pragma unroll
    for (int k = 0; k < 4; k++) r.c[k] = mip_cubic_value(p0.c[k], p1.c[k], p2.c[k], p3.c[k], x);
    return r;
}

// ---- host: the triangle filter's lists ----------------------------------------------------------------------------------------------

// one entry of TriangleFilter::_Create's output: source texel `from` adds weight * texel to destination `to`
struct MipTriEntry { int32_t from, to; float weight; };

// TriangleFilter::_Create(source, dest, wrap), restated: the entries of every source index in the order the reference stores them
inline void mip_triangle_lists(int32_t source, int32_t dest, bool wrap, std::vector<MipTriEntry>& out)
{
    out.clear();
    const float scale = (float)dest / (float)source;
    const float scaleInv = 0.5f / scale;
    int64_t accumU = 0;                                           // (the reference never resets it between source indices)
    float accumWeight = 0.f;
    for (int32_t u = 0; u < source; ++u) {
        for (int j = 0; j < 2; ++j) {
            const float src = (float)(u + j) - 0.5f;
            float destMin = src * scale;
            float destMax = destMin + scale;
            if (!wrap) {
                if (destMin < 0.f) destMin = 0.f;
                if (destMax > (float)dest) destMax = (float)dest;
            }
            for (int64_t k = (int64_t)floorf(destMin); (float)k < destMax; ++k) {
                float d0 = (float)k;
                float d1 = d0 + 1.f;
                int64_t u0;
                if (k < 0) u0 = k + dest;
                else if (k >= dest) u0 = k - dest;
                else u0 = k;
                if (u0 != accumU) {
                    if (accumWeight > 0.00001f) out.push_back(MipTriEntry{u, (int32_t)accumU, accumWeight});
                    accumWeight = 0.f;
                    accumU = u0;
                }
                if (d0 < destMin) d0 = destMin;
                if (d1 > destMax) d1 = destMax;
                float weight;
                if (!wrap && src < 0.f) weight = 1.f;
                else if (!wrap && ((src + 1.f) >= (float)source)) weight = 0.f;
                else { weight = (d0 + d1) * scaleInv; weight = weight - src; }
                const float span = d1 - d0;
                const float part = span * (j ? (1.f - weight) : weight);
                accumWeight = accumWeight + part;
            }
        }
        if (accumWeight > 0.00001f) out.push_back(MipTriEntry{u, (int32_t)accumU, accumWeight});
        accumWeight = 0.f;
    }
}

// The lists inverted for a gather, order preserved: words[0 .. dest] are the first entry of each destination (relative to words + dest + 1,
// in entries), then per entry two words, the source index and the weight's bits.  A destination's entries keep the reference's order of
// arrival: sources ascending, a source's own entries as stored.  Appends to `words`; returns false where a destination is outside 0 .. dest-1.
// *repeats becomes true where one source reaches one destination through two entries (a wrap fold can do that): only then does the
// order of arrival in two dimensions differ from rows outside, columns inside.
inline bool mip_triangle_gather(const std::vector<MipTriEntry>& lists, int32_t dest, std::vector<uint32_t>& words, bool* repeats)
{
    const size_t base = words.size();
    words.resize(base + (size_t)dest + 1 + 2 * lists.size(), 0u);
    uint32_t* start = words.data() + base;
    for (const MipTriEntry& e : lists) {
        if (e.to < 0 || e.to >= dest) return false;
        start[e.to + 1]++;
    }
    for (int32_t d = 0; d < dest; d++) start[d + 1] += start[d];
    std::vector<uint32_t> at(start, start + dest);
    uint32_t* ent = start + dest + 1;
    for (const MipTriEntry& e : lists) {                          // stable: ascending sources, list order within one
        const uint32_t i = at[(size_t)e.to]++;
        uint32_t bits;
        memcpy(&bits, &e.weight, 4);
        ent[2 * i] = (uint32_t)e.from;
        ent[2 * i + 1] = bits;
        if (i > start[e.to] && ent[2 * (i - 1)] == (uint32_t)e.from) *repeats = true;
    }
    return true;
}

} // namespace itw
