// height_normal_core.hpp -- a height map to a tangent-space normal map, per texel: DirectXTex's ComputeNormalMap (DirectXTexNormalMaps.cpp:22-244
// _EvaluateColor, _EvaluateRow, _ComputeNMap) restated for one texel and its eight neighbours.  Plain C++ under a few macros, as bc1a_core.hpp:
// the same text is the kernel's (height_normal.hip, which explains the mapping) and a host program's (tools/height_normal_host_check.cpp walks
// images through it on the CPU).  IEEE fp32, every operation rounded on its own: build with -ffp-contract=off, correctly rounded divide and
// square root.  include/itw_dispatch.h ("height maps") is the contract; the `ops` word's layout is restated below.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define HN_FN __host__ __device__ __forceinline__
#define HN_UNROLL _Pragma("unroll")
#else
#define HN_FN inline
#define HN_UNROLL
#endif

namespace itw {
namespace hn {

// the `ops` word (ITW_NORMAL_FROM_HEIGHT, ITW_HEIGHT_*): every bit above 7 counts only together with FROM_HEIGHT
constexpr uint32_t FROM_HEIGHT = 0x20u, CHANNEL_MASK = 0xF00u, MIRROR_U = 0x1000u, MIRROR_V = 0x2000u, INVERT_SIGN = 0x4000u, OCCLUSION = 0x8000u,
                   AMPLITUDE_MASK = 0x7FFF0000u;
constexpr int CHANNEL_SHIFT = 8, AMPLITUDE_SHIFT = 16;
constexpr uint32_t OPS_KNOWN = 7u | FROM_HEIGHT | CHANNEL_MASK | MIRROR_U | MIRROR_V | INVERT_SIGN | OCCLUSION | AMPLITUDE_MASK;
constexpr uint32_t CHANNEL_LUMINANCE = 5u;                        // 0 and 1 red, 2 green, 3 blue, 4 alpha (CNMAP_CHANNEL_*)

HN_FN uint32_t ops_channel(uint32_t ops) { return (ops & CHANNEL_MASK) >> CHANNEL_SHIFT; }
HN_FN uint32_t ops_amplitude_bits(uint32_t ops) { return (ops & AMPLITUDE_MASK) >> AMPLITUDE_SHIFT; }

// what is wrong with an `ops` word, first fault first; `ops <= 7` is the word of the calls as they were
enum OpsFault { OPS_OK = 0, OPS_UNKNOWN_BITS, OPS_CHANNEL, OPS_AMPLITUDE };
HN_FN OpsFault ops_fault(uint32_t ops)
{
    if (!(ops & FROM_HEIGHT)) return (ops & ~7u) ? OPS_UNKNOWN_BITS : OPS_OK;
    if (ops & ~OPS_KNOWN) return OPS_UNKNOWN_BITS;
    if (ops_channel(ops) > CHANNEL_LUMINANCE) return OPS_CHANNEL;
    const uint32_t a = ops_amplitude_bits(ops);
    if (a == 0u || a >= 0x7C00u) return OPS_AMPLITUDE;            // zero, infinite or NaN: the amplitude is a finite half above 0
    return OPS_OK;
}

// the texel kinds a height is read from and a normal is stored to.  DST_HALF_SIGNED: RGBA16F in the signed convention (a flip negates);
// DST_FLOAT: the unrounded normal (the host check's only)
enum Src { SRC_UNORM8 = 0, SRC_SNORM8 = 1, SRC_HALF = 2, SRC_FLOAT = 3 };
enum Dst { DST_RGBA8 = 0, DST_SNORM8 = 1, DST_HALF = 2, DST_HALF_SIGNED = 3, DST_FLOAT = 4 };
template <int SRC> struct SrcBytes { static constexpr int value = SRC == SRC_FLOAT ? 16 : SRC == SRC_HALF ? 8 : 4; };
template <int DST> struct DstBytes { static constexpr int value = DST == DST_FLOAT ? 16 : (DST == DST_HALF || DST == DST_HALF_SIGNED) ? 8 : 4; };

HN_FN float bits_float(uint32_t u) { float f; memcpy(&f, &u, sizeof f); return f; }
HN_FN uint32_t float_bits(float f) { uint32_t u; memcpy(&u, &f, sizeof u); return u; }

// a half widened exactly
HN_FN float half_float(uint32_t h)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __half2float(__ushort_as_half((unsigned short)h));
#else
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    if (e == 31u) return bits_float(sign | 0x7f800000u | (m << 13));
    if (e != 0u) return bits_float(sign | ((e + 112u) << 23) | (m << 13));
    const float v = (float)m * 5.9604644775390625e-8f;            // m * 2^-24: exact
    return sign ? -v : v;
#endif
}

// the RGBA16F store, the mip filter's rule (mipgen.hpp mip_half_bits): NaN -> 0x7E00, clamp to +-65504, round to nearest even.  On the device
// the value passes through an empty asm in front of the conversion, normal_prep.hpp's device: whatever produced it is not fused into
// v_fma_mixlo_f16 x, y, +0, which would lose the sign of a -0
HN_FN uint32_t half_bits(float v)
{
    if (v != v) return 0x7e00u;
    v = fminf(fmaxf(v, -65504.0f), 65504.0f);
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(v));
    return (uint32_t)__half_as_ushort(__float2half_rn(v));
#else
    const uint32_t u = float_bits(v), sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a < 0x33000001u) return sign;                             // at most 2^-25: the tie goes to the even 0
    if (a < 0x38800000u) {                                        // below 2^-14: a denormal half, units of 2^-24
        const int shift = 126 - (int)(a >> 23);                   // 14 .. 24
        const uint32_t m = (a & 0x7fffffu) | 0x800000u;
        uint32_t q = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
        if (rem > half || (rem == half && (q & 1u))) q++;
        return sign | q;
    }
    uint32_t q = (a - 0x38000000u) >> 13;                         // exponent and mantissa in place; a carry runs into the exponent
    const uint32_t rem = a & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (q & 1u))) q++;
    return sign | q;
#endif
}

// one component to its int8 code: normal_prep.hpp's normal_quantize_snorm (NaN -> 0, clamp to [-1, 1], * 127, round to nearest even)
HN_FN int32_t snorm_code(float v)
{
    if (v != v) return 0;
    const float c = fminf(fmaxf(v, -1.0f), 1.0f);
    const float p = c * 127.0f;
    return (int32_t)rintf(p);
}

// one component to its biased 8-bit code, the library's own rule: NaN -> 0, clamp to [0, 1], * 255, + 0.5, truncate.  0.5 is 128, 1 is 255
HN_FN uint32_t unorm_code(float v)
{
    if (v != v) return 0u;
    const float c = fminf(fmaxf(v, 0.0f), 1.0f);
    const float p = c * 255.0f;
    return (uint32_t)(p + 0.5f);
}

// component c of the texel at `p`: the load rules of the four kinds
template <int SRC>
HN_FN float component(const uint8_t* p, int c)
{
    if (SRC == SRC_UNORM8) return (float)p[c] * (1.0f / 255.0f);
    if (SRC == SRC_SNORM8) return fmaxf((float)(int8_t)p[c] * (1.0f / 127.0f), -1.0f);
    if (SRC == SRC_HALF) { uint16_t h; memcpy(&h, __builtin_assume_aligned(p + 2 * c, 2), sizeof h); return half_float(h); }
    float f; memcpy(&f, __builtin_assume_aligned(p + 4 * c, 4), sizeof f); return f;
}

// _EvaluateColor: the height of a texel from its components.  `channel` is uniform over a call
HN_FN float evaluate(float r, float g, float b) { return (r * 0.2125f + g * 0.7154f) + b * 0.0721f; }
template <int SRC>
HN_FN float height_at(const uint8_t* p, uint32_t channel)
{
    if (channel == CHANNEL_LUMINANCE) return evaluate(component<SRC>(p, 0), component<SRC>(p, 1), component<SRC>(p, 2));
    return component<SRC>(p, channel < 2u ? 0 : (int)channel - 1);
}
// the same from the texel's words (8-bit kinds: one word; half: two), for the whole-vector loads of a row quad
template <int SRC>
HN_FN float height_of_words(const uint32_t* w, uint32_t channel)
{
    static_assert(SRC != SRC_FLOAT, "float texels are loaded a component at a time");
    float c[4];
    HN_UNROLL
    for (int k = 0; k < 4; k++) {
        if (SRC == SRC_UNORM8)      c[k] = (float)((w[0] >> (8 * k)) & 255u) * (1.0f / 255.0f);
        else if (SRC == SRC_SNORM8) c[k] = fmaxf((float)((int32_t)(w[0] << (24 - 8 * k)) >> 24) * (1.0f / 127.0f), -1.0f);
        else                        c[k] = half_float((w[k >> 1] >> (16 * (k & 1))) & 0xffffu);
    }
    if (channel == CHANNEL_LUMINANCE) return evaluate(c[0], c[1], c[2]);
    return channel < 2u ? c[0] : channel == 2u ? c[1] : channel == 3u ? c[2] : c[3];
}

// the neighbour of an edge: column (row) -1 or `size`.  Wrap, the reference's default: the opposite edge; mirror: the edge itself
HN_FN int32_t neighbour(int32_t i, int32_t size, bool mirror)
{
    if (i < 0) return mirror ? 0 : size - 1;
    if (i >= size) return mirror ? size - 1 : 0;
    return i;
}

struct Normal { float x, y, z, a; };

// _ComputeNMap's inner loop (:173-227) for one texel: v0, v1, v2 are the heights of rows y - 1, y, y + 1 at columns x - 1, x, x + 1.
// Returns what the reference hands to _StoreScanline: the encoded normal and alpha.  `biased`: a UNORM target (CONVF_UNORM)
HN_FN Normal texel(const float (&v0)[3], const float (&v1)[3], const float (&v2)[3], uint32_t ops, float amplitude, bool biased)
{
    float t = ((v0[0] - v0[2]) + (v1[0] - v1[2])) + (v2[0] - v2[2]);
    const float dzx = (t * amplitude) / 6.0f;
    t = ((v0[0] - v2[0]) + (v0[1] - v2[1])) + (v0[2] - v2[2]);
    const float dzy = (t * amplitude) / 6.0f;

    // XMVector3Cross(vx, vy), the six products and three differences as DirectXMath writes them: the sign of a zero depends on the form
    const float vxx = -1.0f, vxy = 0.0f, vxz = dzx;
    const float vyx = 0.0f, vyy = -1.0f, vyz = dzy;
    const float cx = vxy * vyz - vxz * vyy;
    const float cy = vxz * vyx - vxx * vyz;
    const float cz = vxx * vyy - vxy * vyx;
    // XMVector3Normalize, the SSE form: true divides by the length; an infinite length gives NaN in every component
    const float m = sqrtf((cx * cx + cy * cy) + cz * cz);
    Normal n;
    n.x = cx / m; n.y = cy / m; n.z = cz / m;
    if (m == INFINITY) n.x = n.y = n.z = bits_float(0x7fc00000u);

    float alpha = 1.0f;
    if (ops & OCCLUSION) {                                        // :190-210
        float delta = 0.0f;
        const float c = v1[1];
        float d = v0[0] - c; if (d > 0.0f) delta += d;
        d = v0[1] - c; if (d > 0.0f) delta += d;
        d = v0[2] - c; if (d > 0.0f) delta += d;
        d = v1[0] - c; if (d > 0.0f) delta += d;
        d = v1[2] - c; if (d > 0.0f) delta += d;
        d = v2[0] - c; if (d > 0.0f) delta += d;
        d = v2[1] - c; if (d > 0.0f) delta += d;
        d = v2[2] - c; if (d > 0.0f) delta += d;
        delta *= 0.125f * amplitude;
        if (delta > 0.0f) {
            const float r = sqrtf(1.0f + delta * delta);
            alpha = (r - delta) / r;
        }
    }

    if (biased) {                                                 // XMVectorMultiplyAdd(+-0.5, normal, 0.5): a multiply, then an add
        const float k = (ops & INVERT_SIGN) ? -0.5f : 0.5f;
        n.x = k * n.x + 0.5f; n.y = k * n.y + 0.5f; n.z = k * n.z + 0.5f;
    } else if (ops & INVERT_SIGN) {
        n.x = -n.x; n.y = -n.y; n.z = -n.z;
    }
    n.a = alpha;
    return n;
}

} // namespace hn
} // namespace itw
