// bc3_core.hpp -- the arithmetic of DirectXTex's BC3 encoder: D3DXEncodeBC3 (BC.cpp:939-1139; COLOR_WEIGHTS is not defined there, BC.cpp:19),
// restated for one block in registers.  The alpha half is here -- the quantise-and-diffuse pre-pass, the 6-step or 8-step choice,
// OptimizeAlpha<false> (BC.h:727-856) over the pre-pass's points, the endpoint order and the fDot index rule with its second diffusion --;
// the colour half is EncodeBC1(..., bColorKey = false, 0.f, flags), which bc1a_core.hpp's bc1a_encode computes for alpha_ref = 0.0f without
// its DITHER_A bit (bc2_core.hpp says why).  This is NOT BC4's encoder: BC4 picks the nearest decoded level, BC3 rounds fDot along the ramp,
// so bc4_bc5.hip's run table does not apply, and its Newton loop (LDS weights, a scale carrying 16) is restated here in plain form -- the
// points are floats that may leave [0, 1], not 8-bit codes.  Plain C++ under bc1a_core.hpp's macros, so the same text is the kernel's
// (bc3_dxtex.hip) and a host program's (tools/bc3_host_check.cpp).  fp32 throughout, one rounding per operation: -ffp-contract=off.
#pragma once
#include <cstdint>
#include "bc1a_core.hpp"

namespace itw {
namespace bc3 {

struct Bc3Block { uint32_t alpha0, alpha1, ends, bitmap; };      // alpha[0], alpha[1], bitmap[0..1] | bitmap[2..5] | the BC1 block's two words

// a[k] for a k that is only known at run time, from registers: three levels of selects, no indexed array (no scratch)
BC1A_FN float bc3_pick(const float (&a)[8], uint32_t k)
{
    const float p0 = (k & 1u) ? a[1] : a[0], p1 = (k & 1u) ? a[3] : a[2], p2 = (k & 1u) ? a[5] : a[4], p3 = (k & 1u) ? a[7] : a[6];
    const float q0 = (k & 2u) ? p1 : p0, q1 = (k & 2u) ? p3 : p2;
    return (k & 4u) ? q1 : q0;
}

// OptimizeAlpha<false> (BC.h:727-856) over the sixteen points p[], which need not lie in [0, 1].  six: cSteps == 6.
BC1A_FN void bc3_optimize_alpha(float& outx, float& outy, const float (&p)[16], bool six)
{
    // pC6 / pD6 / pC8 / pD8 as the source's tables hold them: the quotients k / 5 and k / 7; entries 6, 7 of the 6-step tables are never read
    float c[8], d[8];
    c[0] = 1.0f;                       d[0] = 0.0f;
    c[1] = six ? 4.0f / 5.0f : 6.0f / 7.0f; d[1] = six ? 1.0f / 5.0f : 1.0f / 7.0f;
    c[2] = six ? 3.0f / 5.0f : 5.0f / 7.0f; d[2] = six ? 2.0f / 5.0f : 2.0f / 7.0f;
    c[3] = six ? 2.0f / 5.0f : 4.0f / 7.0f; d[3] = six ? 3.0f / 5.0f : 3.0f / 7.0f;
    c[4] = six ? 1.0f / 5.0f : 3.0f / 7.0f; d[4] = six ? 4.0f / 5.0f : 4.0f / 7.0f;
    c[5] = six ? 0.0f / 5.0f : 2.0f / 7.0f; d[5] = six ? 5.0f / 5.0f : 5.0f / 7.0f;
    c[6] = six ? 0.0f : 1.0f / 7.0f;        d[6] = six ? 0.0f : 6.0f / 7.0f;
    c[7] = 0.0f;                            d[7] = six ? 0.0f : 1.0f;

    float fx = 1.0f, fy = 0.0f;
BC1A_UNROLL
    for (int i = 0; i < 16; i++) {
        if (six) {                                                 // the start values leave out the points the codes 6 and 7 serve
            if (p[i] < fx && p[i] > 0.0f) fx = p[i];
            if (p[i] > fy && p[i] < 1.0f) fy = p[i];
        } else {
            if (p[i] < fx) fx = p[i];
            if (p[i] > fy) fy = p[i];
        }
    }
    if (six && fx == fy) fy = 1.0f;

    const float fsteps = six ? 5.0f : 7.0f;
    const uint32_t csteps = six ? 6u : 8u;
BC1A_NOUNROLL
    for (int it = 0; it < 8; it++) {
        if ((fy - fx) < (1.0f / 256.0f)) break;
        const float scale = fsteps / (fy - fx);
        // pSteps[k] = pC[k] * fX + pD[k] * fY (6 steps: [6], [7] are not read).  Written out, not looped: an array that a loop fills is still
        // memory when the selects of bc3_pick are formed, and the compiler then indexes it (LDS) instead of selecting registers
        const float s[8] = {c[0] * fx + d[0] * fy, c[1] * fx + d[1] * fy, c[2] * fx + d[2] * fy, c[3] * fx + d[3] * fy,
                            c[4] * fx + d[4] * fy, c[5] * fx + d[5] * fy, c[6] * fx + d[6] * fy, c[7] * fx + d[7] * fy};
        const float to_zero = fx * 0.5f, to_one = (fy + 1.0f) * 0.5f;
        float dx = 0.0f, dy = 0.0f, d2x = 0.0f, d2y = 0.0f;
BC1A_UNROLL
        for (int i = 0; i < 16; i++) {
            const float dot = (p[i] - fx) * scale;
            uint32_t k;
            if (dot <= 0.0f) k = (six && p[i] <= to_zero) ? 6u : 0u;
            else if (dot >= fsteps) k = (six && p[i] >= to_one) ? 7u : csteps - 1u;
            else k = (uint32_t)(int32_t)(dot + 0.5f);
            if (k < csteps) {
                const float ck = bc3_pick(c, k), dk = bc3_pick(d, k);
                const float diff = bc3_pick(s, k) - p[i];
                dx += ck * diff;
                d2x += ck * ck;
                dy += dk * diff;
                d2y += dk * dk;
            }
        }
        if (d2x > 0.0f) fx -= dx / d2x;
        if (d2y > 0.0f) fy -= dy / d2y;
        if (fx > fy) { const float f = fx; fx = fy; fy = f; }
        if ((dx * dx < (1.0f / 64.0f)) && (dy * dy < (1.0f / 64.0f))) break;
    }
    outx = (fx < 0.0f) ? 0.0f : (fx > 1.0f) ? 1.0f : fx;
    outy = (fy < 0.0f) ? 0.0f : (fy > 1.0f) ? 1.0f : fy;
}

// The alpha half (BC.cpp:952-1003, 1018-1138): a0 = alpha[0] | alpha[1] << 8 | bitmap[0..1] << 16, a1 = bitmap[2..5].
template <bool DITHER_A>
BC1A_FN void bc3_alpha(const uint32_t (&w)[16], uint32_t& a0, uint32_t& a1)
{
    // ---- the pre-pass: the points are the alphas rounded to 8 bits -- with DITHER_A after the diffused error was added, so a point may fall
    // below 0 (the cast truncates toward zero) or rise above 1.  The minimum and maximum start from texel 0's UNROUNDED alpha, and a point
    // that lowers the minimum is not looked at for the maximum (`else if`).
    float pt[16];
    float fmin = (float)(w[0] >> 24) * bc1a::BC1A_UNORM, fmax = fmin;
    {
        float e[16];
        if (DITHER_A) {
BC1A_UNROLL
            for (int i = 0; i < 16; i++) e[i] = 0.0f;
        }
BC1A_UNROLL
        for (int i = 0; i < 16; i++) {
            float alph = (float)(w[i] >> 24) * bc1a::BC1A_UNORM;
            if (DITHER_A) alph += e[i];
            pt[i] = (float)(int32_t)(alph * 255.0f + 0.5f) * (1.0f / 255.0f);
            if (pt[i] < fmin) fmin = pt[i];
            else if (pt[i] > fmax) fmax = pt[i];
            if (DITHER_A) bc1a::bc1a_diffuse(e, i, alph - pt[i]);
        }
    }
    if (1.0f == fmin) { a0 = 0xffffu; a1 = 0u; return; }           // all opaque: FF FF and a zero bitmap

    const bool six = (0.0f == fmin) || (1.0f == fmax);
    float fa, fb;
    bc3_optimize_alpha(fa, fb, pt, six);
    const uint32_t ba = (uint32_t)(int32_t)(fa * 255.0f + 0.5f) & 0xffu, bb = (uint32_t)(int32_t)(fb * 255.0f + 0.5f) & 0xffu;
    fa = (float)ba * (1.0f / 255.0f);
    fb = (float)bb * (1.0f / 255.0f);
    if (!six && ba == bb) { a0 = ba | (bb << 8); a1 = 0u; return; }

    // ---- the steps: 6 steps store (A, B) and end in the codes for exactly 0 and exactly 1, 8 steps store (B, A)
    const float s0 = six ? fa : fb, s1 = six ? fb : fa;
    const uint32_t ends = six ? (ba | (bb << 8)) : (bb | (ba << 8));
    // fStep[i + 1] = (fStep[0] * (n - i) + fStep[1] * i) * (1 / n), n = 5 or 7; 6 steps: [6] = 0.0f, [7] = 1.0f (written out: see above)
    const float st[8] = {s0, s1,
                         six ? (s0 * 4.0f + s1 * 1.0f) * (1.0f / 5.0f) : (s0 * 6.0f + s1 * 1.0f) * (1.0f / 7.0f),
                         six ? (s0 * 3.0f + s1 * 2.0f) * (1.0f / 5.0f) : (s0 * 5.0f + s1 * 2.0f) * (1.0f / 7.0f),
                         six ? (s0 * 2.0f + s1 * 3.0f) * (1.0f / 5.0f) : (s0 * 4.0f + s1 * 3.0f) * (1.0f / 7.0f),
                         six ? (s0 * 1.0f + s1 * 4.0f) * (1.0f / 5.0f) : (s0 * 3.0f + s1 * 4.0f) * (1.0f / 7.0f),
                         six ? 0.0f : (s0 * 2.0f + s1 * 5.0f) * (1.0f / 7.0f),
                         six ? 1.0f : (s0 * 1.0f + s1 * 6.0f) * (1.0f / 7.0f)};
    const float fsteps = six ? 5.0f : 7.0f;
    const uint32_t last = six ? 5u : 7u;
    const float scale = (st[0] != st[1]) ? (fsteps / (st[1] - st[0])) : 0.0f;
    const float to_zero = st[0] * 0.5f, to_one = (st[1] + 1.0f) * 0.5f;

    // ---- the indices, over the SOURCE alpha (a fresh error array with DITHER_A): pSteps6 = {0, 2, 3, 4, 5, 1}, pSteps8 = {0, 2, 3, 4, 5, 6, 7, 1}
    float e[16];
    if (DITHER_A) {
BC1A_UNROLL
        for (int i = 0; i < 16; i++) e[i] = 0.0f;
    }
    uint32_t dw[2] = {0u, 0u};
BC1A_UNROLL
    for (int i = 0; i < 16; i++) {
        float alph = (float)(w[i] >> 24) * bc1a::BC1A_UNORM;
        if (DITHER_A) alph += e[i];
        const float dot = (alph - st[0]) * scale;
        uint32_t step;
        if (dot <= 0.0f) step = (six && alph <= to_zero) ? 6u : 0u;
        else if (dot >= fsteps) step = (six && alph >= to_one) ? 7u : 1u;
        else { const uint32_t k = (uint32_t)(int32_t)(dot + 0.5f); step = k == 0u ? 0u : k == last ? 1u : k + 1u; }
        dw[i >> 3] = (step << 21) | (dw[i >> 3] >> 3);
        if (DITHER_A) bc1a::bc1a_diffuse(e, i, alph - bc3_pick(st, step));
    }
    a0 = ends | ((dw[0] & 0xffffu) << 16);
    a1 = ((dw[0] >> 16) & 0xffu) | (dw[1] << 8);
}

// One block: w = its sixteen RGBA8 texels (R in the low byte), raster order.  DITHER: bc1a's template bits (BC1A_DITHER_RGB, BC1A_DITHER_A).
// The alpha pass runs first and leaves only its two words, so its arrays are dead before OptimizeRGB starts.
template <uint32_t DITHER>
BC1A_FN Bc3Block bc3_encode(const uint32_t (&w)[16], bool uniform)
{
    Bc3Block o;
    bc3_alpha<(DITHER & bc1a::BC1A_DITHER_A) != 0>(w, o.alpha0, o.alpha1);
    const bc1a::Bc1aBlock c = bc1a::bc1a_encode<(DITHER & bc1a::BC1A_DITHER_RGB)>(w, 0.0f, uniform);
    o.ends = c.ends;
    o.bitmap = c.bitmap;
    return o;
}

} // namespace bc3
} // namespace itw
