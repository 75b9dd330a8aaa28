// mipgen.hpp -- the arithmetic of the mip filters (include/itw_dispatch.h, "Mip chains"): one definition behind the pyramid kernels and the
// per-level kernel of mipgen.hip.  DirectXTex's non-WIC 2D filters (DirectXTexMipmaps.cpp:715-805 box, :809-917 linear; Filters.h:33-39
// AVERAGE4, :66-106 _CreateLinearFilter and BILINEAR_INTERPOLATE) with the R16G16B16A16_FLOAT scanline store (DirectXTexConvert.cpp:1634-1646).
// IEEE fp32, one rounding per operation (the library is built with -ffp-contract=off).  All four channels alike -- but for the sRGB colour
// kind (ITW_MIP_SRGB), the library's own rule: the same filters over R, G, B decoded to linear light, stored as the nearest sRGB code.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include "srgb_tables.h"

namespace itw {

struct MipTexel { float c[4]; };                                  // a stored texel, widened: every value is one the texel format holds

// The sRGB colour kind (ITW_MIP_SRGB; RGBA8 texels whose R, G, B are sRGB coded, A linear): the tables of srgb_tables.h as the kernels hold
// them in LDS.  dec[c] = D[c]; thr[k] = T[k] for k = 1..255, and thr[0] = thr[256] = NaN, which no value is below and none at or above.
struct MipSrgbTables { float dec[256]; float thr[257]; };

// fills `t` from the tables in memory; every lane of a 256-lane workgroup calls it, and it ends with the barrier that publishes the tables
__device__ __forceinline__ void mip_srgb_fill(MipSrgbTables* t)
{
    t->dec[threadIdx.x] = __uint_as_float(SRGB_DECODE_BITS[threadIdx.x]);
    t->thr[threadIdx.x] = __uint_as_float(threadIdx.x ? SRGB_THR_BITS[threadIdx.x] : 0x7fc00000u);
    if (threadIdx.x == 0) t->thr[256] = __uint_as_float(0x7fc00000u);
    __syncthreads();
}

// E(v): the number of k in 1..255 with v >= T[k].  A guess g from the curve's inverse, then one compare either side: E = g - (v < T[g]) +
// (v >= T[g + 1]), which is the count whenever |g - E| <= 1 (T is strictly increasing).  The guess is floor(c + 0.5) of c = 255 * the sRGB
// encoding of v, through v_log_f32 / v_exp_f32 (1 ulp each: c is off by less than 1e-3 codes, the fp32 operations around them included),
// while T[k] is the value whose c is k - 0.5 (to an fp32 ulp of T): g and E round the same number, so they differ by one at the most, and only
// next to a threshold.  tests/test_srgb_mips_cpu.py restates the guess on the host and adds +-0.05 codes of error to c: |g - E| <= 1 holds on
// every float within 4096 ulps of a threshold; tests/test_gpu_srgb_mips.py runs this function on the floats around every T[k].  Values above 1 give 255 (the
// clamp, and NaN above T[255]); -0, 0, negative values and NaN give 0.
__device__ __forceinline__ uint32_t mip_srgb_encode(float v, const MipSrgbTables* t)
{
    float c = v * (12.92f * 255.0f);
    if (v > 0.0031308f) c = 269.025f * __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(v) * (1.0f / 2.4f)) - 14.025f;   // (v_log_f32 is log2; no denormal in or out here)
    const int32_t g = (int32_t)fminf(fmaxf(c + 0.5f, 0.0f), 255.0f);         // (fmaxf(NaN, 0) is 0)
    return (uint32_t)(g - (v < t->thr[g] ? 1 : 0) + (v >= t->thr[g + 1] ? 1 : 0));
}

// PX = 4: RGBA8, the raw codes as 0..255; with SRGB, R, G and B are D[code] and A stays the raw code.  PX = 8: RGBA16F, the halves widened
// exactly.  `srgb` is the workgroup's tables (SRGB only).
template <int PX, bool SRGB = false>
__device__ __forceinline__ MipTexel mip_widen(uint32_t lo, uint32_t hi, const MipSrgbTables* srgb = nullptr)
{
    static_assert(!SRGB || PX == 4, "sRGB colour is an RGBA8 kind");
    MipTexel t;
    if (SRGB) {
        t.c[0] = srgb->dec[lo & 255u]; t.c[1] = srgb->dec[(lo >> 8) & 255u]; t.c[2] = srgb->dec[(lo >> 16) & 255u]; t.c[3] = (float)(lo >> 24);
    } else if (PX == 4) {
        t.c[0] = (float)(lo & 255u); t.c[1] = (float)((lo >> 8) & 255u); t.c[2] = (float)((lo >> 16) & 255u); t.c[3] = (float)(lo >> 24);
    } else {
        t.c[0] = __half2float(__ushort_as_half((unsigned short)(lo & 0xffffu))); t.c[1] = __half2float(__ushort_as_half((unsigned short)(lo >> 16)));
        t.c[2] = __half2float(__ushort_as_half((unsigned short)(hi & 0xffffu))); t.c[3] = __half2float(__ushort_as_half((unsigned short)(hi >> 16)));
    }
    return t;
}

// RGBA16F store: a NaN stores 0x7E00; anything else is clamped to [-65504, 65504] and rounded to nearest even (convert.hip's to_half_bits).
// An exact -0 keeps its sign: the clamp stands between the filter's last multiply and the conversion, so the two are not fused into
// v_fma_mixlo_f16 x, y, +0 as in normal_prep.hpp's trap ((-0) + (+0) is +0).  tests/test_gpu_mipgen.py holds exact -0 sums at every level kind.
__device__ __forceinline__ uint32_t mip_half_bits(float v)
{
    if (v != v) return 0x7e00u;
    v = fminf(fmaxf(v, -65504.0f), 65504.0f);
    return (uint32_t)__half_as_ushort(__float2half_rn(v));
}
// RGBA8 store: (uint8_t)min(v + 0.5f, 255.0f); v is never negative or NaN here (codes and weights are not)
__device__ __forceinline__ uint32_t mip_byte(float v) { return (uint32_t)fminf(v + 0.5f, 255.0f); }
// the same store where a filter has negative lobes (ITW_MIP_CUBIC): (uint8_t)min(max(v, 0.0f) + 0.5f, 255.0f), the rule above for every v >= 0
__device__ __forceinline__ uint32_t mip_byte_signed(float v) { return (uint32_t)fminf(fmaxf(v, 0.0f) + 0.5f, 255.0f); }
template <bool NEG> __device__ __forceinline__ uint32_t mip_byte_kind(float v) { return NEG ? mip_byte_signed(v) : mip_byte(v); }

// rounds `t` to the texel format: the words to store, and `t` becomes what a later load of them widens to; NEG: the values may be negative
// (mip_filters.hip's cubic kind), which changes the raw-code store alone
template <int PX, bool SRGB = false, bool NEG = false>
__device__ __forceinline__ void mip_round(MipTexel& t, uint32_t& lo, uint32_t& hi, const MipSrgbTables* srgb = nullptr)
{
    if (SRGB) {
        lo = mip_srgb_encode(t.c[0], srgb) | (mip_srgb_encode(t.c[1], srgb) << 8) | (mip_srgb_encode(t.c[2], srgb) << 16) | (mip_byte_kind<NEG>(t.c[3]) << 24);
        hi = 0;
    } else if (PX == 4) {
        lo = mip_byte_kind<NEG>(t.c[0]) | (mip_byte_kind<NEG>(t.c[1]) << 8) | (mip_byte_kind<NEG>(t.c[2]) << 16) | (mip_byte_kind<NEG>(t.c[3]) << 24);
        hi = 0;
    } else {
        lo = mip_half_bits(t.c[0]) | (mip_half_bits(t.c[1]) << 16);
        hi = mip_half_bits(t.c[2]) | (mip_half_bits(t.c[3]) << 16);
    }
    t = mip_widen<PX, SRGB>(lo, hi, srgb);
}

// AVERAGE4: p0 = (row 2y, column 2x), p1 = (2y+1, 2x), p2 = (2y, 2x+1), p3 = (2y+1, 2x+1)
__device__ __forceinline__ MipTexel mip_box(const MipTexel& p0, const MipTexel& p1, const MipTexel& p2, const MipTexel& p3)
{
    MipTexel r;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float v = p0.c[k] + p1.c[k];
        v = v + p2.c[k];
        v = v + p3.c[k];
        r.c[k] = v * 0.25f;
    }
    return r;
}

// one axis of _CreateLinearFilter with clamp addressing: `scale` = float(source) / float(dest), computed by the host
struct MipTap { int32_t u0, u1; float w0, w1; };
__device__ __forceinline__ MipTap mip_linear_tap(int32_t u, float scale, int32_t source)
{
    const float srcB = ((float)u + 0.5f) * scale + 0.5f;
    int32_t b = (int32_t)srcB;
    int32_t a = b - 1;
    if (a < 0) a = 0;
    if (b >= source) b = source - 1;
    if (a >= source) a = source - 1;                              // (only where fp32 no longer holds the coordinate, sources of 2^25 texels and more: no read past the row)
    MipTap t;
    t.u0 = a; t.u1 = b;
    t.w0 = 1.0f + (float)b - srcB;
    t.w1 = 1.0f - t.w0;
    return t;
}

// BILINEAR_INTERPOLATE: r00 = row u0 of y, column u0 of x; r01 = same row, column u1; r10, r11 = row u1
__device__ __forceinline__ MipTexel mip_bilinear(const MipTexel& r00, const MipTexel& r01, const MipTexel& r10, const MipTexel& r11, const MipTap& x, const MipTap& y)
{
    MipTexel r;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float top = r00.c[k] * x.w0 + r01.c[k] * x.w1;
        const float bot = r10.c[k] * x.w0 + r11.c[k] * x.w1;
        r.c[k] = y.w0 * top + y.w1 * bot;
    }
    return r;
}

// Alpha-weighted colour (include/itw_dispatch.h, "Mip chains", rule A; RGBA8 kinds): each tap's R, G, B times its alpha code, one fp32
// multiply; the filter as it stands over that and over alpha; then R, G, B divided by the filtered, unrounded alpha, one correctly rounded
// fp32 division (the build passes -fhip-fp32-correctly-rounded-divide-sqrt).  Where that alpha is not above 0 no tap is visible and the
// colour is the plain rule's, formed here from the taps the caller still holds.  Alpha itself is the plain rule's in every case.
__device__ __forceinline__ MipTexel mip_premultiply(const MipTexel& p)
{
    MipTexel r;
    r.c[0] = p.c[0] * p.c[3]; r.c[1] = p.c[1] * p.c[3]; r.c[2] = p.c[2] * p.c[3]; r.c[3] = p.c[3];
    return r;
}
__device__ __forceinline__ void mip_unpremultiply(MipTexel& r, const MipTexel& plain)
{
    const float va = r.c[3];
    if (va > 0.0f) { r.c[0] = r.c[0] / va; r.c[1] = r.c[1] / va; r.c[2] = r.c[2] / va; }
    else           { r.c[0] = plain.c[0]; r.c[1] = plain.c[1]; r.c[2] = plain.c[2]; }
}

// the two filters of either kind: WEIGHT = false is mip_box / mip_bilinear and nothing else
template <bool WEIGHT>
__device__ __forceinline__ MipTexel mip_box_kind(const MipTexel& p0, const MipTexel& p1, const MipTexel& p2, const MipTexel& p3)
{
    if constexpr (!WEIGHT) {
        return mip_box(p0, p1, p2, p3);
    } else {
        MipTexel r = mip_box(mip_premultiply(p0), mip_premultiply(p1), mip_premultiply(p2), mip_premultiply(p3));
        if (r.c[3] > 0.0f) mip_unpremultiply(r, r);
        else               mip_unpremultiply(r, mip_box(p0, p1, p2, p3));
        return r;
    }
}

template <bool WEIGHT>
__device__ __forceinline__ MipTexel mip_bilinear_kind(const MipTexel& r00, const MipTexel& r01, const MipTexel& r10, const MipTexel& r11, const MipTap& x,
                                                      const MipTap& y)
{
    if constexpr (!WEIGHT) {
        return mip_bilinear(r00, r01, r10, r11, x, y);
    } else {
        MipTexel r = mip_bilinear(mip_premultiply(r00), mip_premultiply(r01), mip_premultiply(r10), mip_premultiply(r11), x, y);
        if (r.c[3] > 0.0f) mip_unpremultiply(r, r);
        else               mip_unpremultiply(r, mip_bilinear(r00, r01, r10, r11, x, y));
        return r;
    }
}

} // namespace itw
