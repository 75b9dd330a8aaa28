// normal_prep.hpp -- the plugin's normal-map stages, per texel (IntelPlugin.cpp:1506-1545 FlipXYChannelNormalMap, :1550-1613
// NormalizeNormalMapChain): the one definition behind itwPrepareNormalMapChain (normal_prep.hip), the chain gather (chain.hip) and the
// fused BC5 load (bc4_bc5.hip).  The flips come first, then the normalise -- the save path's order (:2103-2106, :2149-2152).  Alpha is
// never touched, blue only by the normalise.  IEEE fp32, one rounding per operation (the library is built with -ffp-contract=off and the
// correctly rounded divide / square root).
// Below them, the signed normal sources (int8, half or float texels to RGBA8_SNORM codes): a second convention with one definition of its own.
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

// ---- signed normal sources (include/itw_dispatch.h, "signed normal sources": the contract) -------------------------------------------------
// A texel of texel_bytes TB -- 4 RGBA8_SNORM, 8 RGBA16F, 16 RGBA32F -- becomes the float vector v = (x, y, z, a); the flips and the normalise
// work on it in fp32 and every component is quantised to an int8 code.  One load per kind, one arithmetic for all three: the one definition
// behind itwQuantizeNormalMapChain (normal_prep.hip), the chain gather of signed sources (chain.hip), the fused BC5_SNORM load (bc4_bc5.hip)
// and, for its loads, the widening of itwCompressSignedNormalMapMipped (mipgen.hip).

// RGBA8_SNORM: one texel word; an int8 code c is max((float)c * (1/127), -1) (itw_bc45.h)
__device__ __forceinline__ void normal_load_rgba8s(float (&v)[4], uint32_t w)
{
#pragma unroll
    for (int c = 0; c < 4; c++) v[c] = fmaxf((float)((int32_t)(w << (24 - 8 * c)) >> 24) * (1.0f / 127.0f), -1.0f);
}
// RGBA16F: lo = R | G << 16, hi = B | A << 16, widened exactly
__device__ __forceinline__ void normal_load_rgba16f(float (&v)[4], uint32_t lo, uint32_t hi)
{
    v[0] = normal_half_to_float(lo & 0xffffu); v[1] = normal_half_to_float(lo >> 16);
    v[2] = normal_half_to_float(hi & 0xffffu); v[3] = normal_half_to_float(hi >> 16);
}
// RGBA32F: as it is
__device__ __forceinline__ void normal_load_rgba32f(float (&v)[4], uint32_t x, uint32_t y, uint32_t z, uint32_t a)
{
    v[0] = __uint_as_float(x); v[1] = __uint_as_float(y); v[2] = __uint_as_float(z); v[3] = __uint_as_float(a);
}
// the texel whose TB / 4 words start at w
template <int TB>
__device__ __forceinline__ void normal_load_signed(float (&v)[4], const uint32_t* w)
{
    static_assert(TB == 4 || TB == 8 || TB == 16, "RGBA8_SNORM, RGBA16F or RGBA32F");
    if (TB == 4)      normal_load_rgba8s(v, w[0]);
    else if (TB == 8) normal_load_rgba16f(v, w[0], w[1]);
    else              normal_load_rgba32f(v, w[0], w[1], w[2], w[3]);
}

// the flips, then the normalise: normal_prep_rgba16f's arithmetic without the rounding to half.  A zero or NaN length gives (0, 0, 1)
__device__ __forceinline__ void normal_signed_ops(float (&v)[4], uint32_t ops)
{
    if (ops & NORMAL_FLIP_X) v[0] = -v[0];
    if (ops & NORMAL_FLIP_Y) v[1] = -v[1];
    if (ops & NORMAL_NORMALIZE) {
        const float x = v[0], y = v[1], z = v[2];
        const float m = sqrtf((x * x + y * y) + z * z);
        v[0] = 0.0f; v[1] = 0.0f; v[2] = 1.0f;
        if (m > 0.0f) {
            const float s = 1.0f / m;
            v[0] = x * s; v[1] = y * s; v[2] = z * s;
        }
    }
}

// one component to its int8 code, -127 .. 127: NaN -> 0, clamp to [-1, 1], * 127, round to nearest even
__device__ __forceinline__ int32_t normal_quantize_snorm(float v)
{
    if (v != v) return 0;
    const float c = fminf(fmaxf(v, -1.0f), 1.0f);
    const float p = c * 127.0f;
    return (int32_t)rintf(p);
}

// a loaded texel through the ops to its RGBA8_SNORM word (R in the low byte)
__device__ __forceinline__ uint32_t normal_quantize_texel(float (&v)[4], uint32_t ops)
{
    normal_signed_ops(v, ops);
    return ((uint32_t)normal_quantize_snorm(v[0]) & 255u) | (((uint32_t)normal_quantize_snorm(v[1]) & 255u) << 8)
         | (((uint32_t)normal_quantize_snorm(v[2]) & 255u) << 16) | ((uint32_t)normal_quantize_snorm(v[3]) << 24);
}

} // namespace itw
