// normal_prep.hpp -- the plugin's normal-map stages, per texel (IntelPlugin.cpp:1506-1545 FlipXYChannelNormalMap, :1550-1613
// NormalizeNormalMapChain): the one definition behind itwPrepareNormalMapChain (normal_prep.hip), the chain gather (chain.hip) and the
// fused BC5 load (bc4_bc5.hip).  The flips come first, then the normalise -- the save path's order (:2103-2106, :2149-2152).  Alpha is
// never touched, blue only by the normalise.  IEEE fp32, one rounding per operation (the library is built with -ffp-contract=off and the
// correctly rounded divide / square root).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

namespace itw {

constexpr uint32_t NORMAL_FLIP_X = 1u, NORMAL_FLIP_Y = 2u, NORMAL_NORMALIZE = 4u, NORMAL_OPS_ALL = 7u;    // ITW_NORMAL_* (itw_dispatch.h)

// RGBA8: one texel word (R in the low byte)
__device__ __forceinline__ uint32_t normal_prep_rgba8(uint32_t w, uint32_t ops)
{
    if (ops & NORMAL_FLIP_X) w ^= 0x000000ffu;                    // 255 - R
    if (ops & NORMAL_FLIP_Y) w ^= 0x0000ff00u;                    // 255 - G
    if (ops & NORMAL_NORMALIZE) {
        const float r = (float)((int32_t)(w & 255u) - 128);
        const float g = (float)((int32_t)((w >> 8) & 255u) - 128);
        const float b = (float)((int32_t)((w >> 16) & 255u) - 128);
        const float m = sqrtf((r * r + g * g) + b * b);
        uint32_t rgb = 0x00ff8080u;                               // the default normal (0, 0, 1): (128, 128, 255)
        if (m > 0.0f) {
            const float s = 127.0f / m;
            rgb = ((uint32_t)(r * s + 128.0f) & 255u) | (((uint32_t)(g * s + 128.0f) & 255u) << 8) | (((uint32_t)(b * s + 128.0f) & 255u) << 16);
        }
        w = (w & 0xff000000u) | rgb;
    }
    return w;
}

__device__ __forceinline__ float normal_half_to_float(uint32_t h) { return __half2float(__ushort_as_half((unsigned short)h)); }
__device__ __forceinline__ uint32_t normal_float_to_half(float v) { return (uint32_t)__half_as_ushort(__float2half_rn(v)); }    // convert.hip to_half_bits
// half(a * b), the product rounded to fp32 first.  The product passes through an empty asm: left to itself the compiler fuses the multiply and
// the conversion into v_fma_mixlo_f16 a, b, +0, and (-0) + (+0) is +0 -- a normal with a -0 component would lose the sign of its zero.
__device__ __forceinline__ uint32_t normal_product_to_half(float a, float b)
{
    float p = a * b;
    asm volatile("" : "+v"(p));
    return normal_float_to_half(p);
}

// RGBA16F: one texel as two words, lo = R | G << 16, hi = B | A << 16
__device__ __forceinline__ void normal_prep_rgba16f(uint32_t& lo, uint32_t& hi, uint32_t ops)
{
    if (ops & NORMAL_FLIP_X) lo = (lo & 0xffff0000u) | normal_float_to_half(1.0f - normal_half_to_float(lo & 0xffffu));
    if (ops & NORMAL_FLIP_Y) lo = (lo & 0x0000ffffu) | (normal_float_to_half(1.0f - normal_half_to_float(lo >> 16)) << 16);
    if (ops & NORMAL_NORMALIZE) {
        const float r = normal_half_to_float(lo & 0xffffu), g = normal_half_to_float(lo >> 16), b = normal_half_to_float(hi & 0xffffu);
        const float m = sqrtf((r * r + g * g) + b * b);
        uint32_t rg = 0u, bb = 0x3c00u;                           // the default normal: (0, 0, 1)
        if (m > 0.0f) {                                           // (false for a NaN length, as in the reference)
            const float s = 1.0f / m;
            rg = normal_product_to_half(r, s) | (normal_product_to_half(g, s) << 16);
            bb = normal_product_to_half(b, s);
        }
        lo = rg;
        hi = (hi & 0xffff0000u) | bb;
    }
}

} // namespace itw
