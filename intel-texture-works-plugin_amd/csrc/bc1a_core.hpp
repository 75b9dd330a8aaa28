// bc1a_core.hpp -- the arithmetic of the BC1-with-1-bit-alpha encoder: DirectXTex's D3DXEncodeBC1 -> EncodeBC1(bColorKey = true) -> OptimizeRGB
// (BC.cpp:67-318, 372-677, 729-787; COLOR_WEIGHTS is not defined there), restated for one block in registers.  Plain C++ under a few macros,
// so the same text is the kernel's (bc1a.hip, which explains the mapping) and a host program's (tools/bc1a_host_check.cpp walks blocks through
// it on the CPU against the reference's own function).  fp32 throughout, one rounding per operation: build with -ffp-contract=off, denormals
// unflushed, correctly rounded divides.
#pragma once
#include <cfloat>
#include <cstdint>

#ifdef __HIPCC__
#define BC1A_FN __host__ __device__ __forceinline__
#define BC1A_UNROLL _Pragma("unroll")           /* every array below is indexed by unrolled loop counters: registers, no scratch */
#define BC1A_NOUNROLL _Pragma("nounroll")
#else
#define BC1A_FN inline
#define BC1A_UNROLL
#define BC1A_NOUNROLL
#endif

namespace itw {
namespace bc1a {

struct Bc1aBlock { uint32_t ends, bitmap; };     // rgb[0] | rgb[1] << 16, the sixteen 2-bit indices
BC1A_FN Bc1aBlock bc1a_block(uint32_t ends, uint32_t bitmap) { Bc1aBlock b; b.ends = ends; b.bitmap = bitmap; return b; }

constexpr float BC1A_UNORM = 1.0f / 255.0f;                       // XMLoadUByteN4's SSE path: integer * (1/255), as bc4_bc5.hip
constexpr float BC1A_LUM_R = 0.2125f / 0.7154f, BC1A_LUM_B = 0.0721f / 0.7154f;       // g_Luminance (fp32 quotients folded at compile time)
constexpr float BC1A_INV_R = 0.7154f / 0.2125f, BC1A_INV_B = 0.7154f / 0.0721f;       // g_LuminanceInv
constexpr uint32_t BC1A_DITHER_RGB = 1u, BC1A_DITHER_A = 2u;      // the kernel's template bits

struct Rgb { float r, g, b; };

// Floyd-Steinberg inside the block (BC.cpp:447-477, 645-671, 754-773): texel i's difference to the right, lower left, below, lower right.
// `i` is a constant once the caller's loop is unrolled.
BC1A_FN void bc1a_diffuse(float (&e)[16], int i, float diff)
{
    if (3 != (i & 3)) e[(i + 1) & 15] += diff * (7.0f / 16.0f);
    if (i < 12) {
        if (i & 3) e[(i + 3) & 15] += diff * (3.0f / 16.0f);
        e[(i + 4) & 15] += diff * (5.0f / 16.0f);
        if (3 != (i & 3)) e[(i + 5) & 15] += diff * (1.0f / 16.0f);
    }
}

// pPoints[i] of OptimizeRGB: the 5:6:5 point of the first pass, times the luminance weights (lg is 1.0f: the identity)
template <bool BIASED>
BC1A_FN Rgb bc1a_point(uint32_t q, float lr, float lb)
{
    float r = (float)(q & 0xffu), g = (float)((q >> 8) & 0xffu), b = (float)((q >> 16) & 0xffu);
    if (BIASED) { r -= 4.0f; g -= 4.0f; b -= 4.0f; }              // exact
    Rgb p;
    p.r = r * (1.0f / 31.0f) * lr;
    p.g = g * (1.0f / 63.0f);
    p.b = b * (1.0f / 31.0f) * lb;
    return p;
}

BC1A_FN uint32_t bc1a_encode565(Rgb c)
{
    c.r = (c.r < 0.0f) ? 0.0f : (c.r > 1.0f) ? 1.0f : c.r;
    c.g = (c.g < 0.0f) ? 0.0f : (c.g > 1.0f) ? 1.0f : c.g;
    c.b = (c.b < 0.0f) ? 0.0f : (c.b > 1.0f) ? 1.0f : c.b;
    return (uint32_t)(((int32_t)(c.r * 31.0f + 0.5f) << 11) | ((int32_t)(c.g * 63.0f + 0.5f) << 5) | (int32_t)(c.b * 31.0f + 0.5f)) & 0xffffu;
}

BC1A_FN Rgb bc1a_decode565(uint32_t w)
{
    Rgb c;
    c.r = (float)((w >> 11) & 31u) * (1.0f / 31.0f);
    c.g = (float)((w >> 5) & 63u) * (1.0f / 63.0f);
    c.b = (float)(w & 31u) * (1.0f / 31.0f);
    return c;
}

BC1A_FN Rgb bc1a_lerp(const Rgb& a, const Rgb& b, float s)
{
    Rgb o;
    o.r = a.r + s * (b.r - a.r);
    o.g = a.g + s * (b.g - a.g);
    o.b = a.b + s * (b.b - a.b);
    return o;
}

// One block: w = its sixteen RGBA8 texels (R in the low byte), raster order.  Returns {rgb[0] | rgb[1] << 16, bitmap}.
template <uint32_t DITHER>
BC1A_FN Bc1aBlock bc1a_encode(const uint32_t (&w)[16], float alpha_ref, bool uniform)
{
    constexpr bool DRGB = (DITHER & BC1A_DITHER_RGB) != 0, DA = (DITHER & BC1A_DITHER_A) != 0;
    const float lr = uniform ? 1.0f : BC1A_LUM_R, lb = uniform ? 1.0f : BC1A_LUM_B;
    const float ir = uniform ? 1.0f : BC1A_INV_R, ib = uniform ? 1.0f : BC1A_INV_B;

    // ---- D3DXEncodeBC1: the alpha the key test sees (with DITHER_A the diffused, rounded one), as a mask: bit i = texel i is transparent
    uint32_t key = 0;
    if (DA) {
        float e[16];
BC1A_UNROLL
        for (int i = 0; i < 16; i++) e[i] = 0.0f;
BC1A_UNROLL
        for (int i = 0; i < 16; i++) {
            const float a = (float)(w[i] >> 24) * BC1A_UNORM;
            const float alph = a + e[i];
            const float q = (float)(int32_t)(a + e[i] + 0.5f);
            key |= (q < alpha_ref ? 1u : 0u) << i;
            bc1a_diffuse(e, i, alph - q);
        }
    } else {
BC1A_UNROLL
        for (int i = 0; i < 16; i++) key |= ((float)(w[i] >> 24) * BC1A_UNORM < alpha_ref ? 1u : 0u) << i;
    }
    if (key == 0xffffu) return bc1a_block(0xffff0000u, 0xffffffffu);
    const bool three = key != 0;                                   // uSteps == 3

    // ---- EncodeBC1, first pass: quantise to 5:6:5 (error diffusion with DITHER_RGB); the points are kept as packed integers
    uint32_t q[16];
    {
        float er[16], eg[16], eb[16];
        if (DRGB) {
BC1A_UNROLL
            for (int i = 0; i < 16; i++) er[i] = eg[i] = eb[i] = 0.0f;
        }
BC1A_UNROLL
        for (int i = 0; i < 16; i++) {
            float r = (float)(w[i] & 0xffu) * BC1A_UNORM, g = (float)((w[i] >> 8) & 0xffu) * BC1A_UNORM, b = (float)((w[i] >> 16) & 0xffu) * BC1A_UNORM;
            if (DRGB) { r += er[i]; g += eg[i]; b += eb[i]; }
            const int32_t qr = (int32_t)(r * 31.0f + 0.5f), qg = (int32_t)(g * 63.0f + 0.5f), qb = (int32_t)(b * 31.0f + 0.5f);   // toward zero
            constexpr int32_t B = DRGB ? 4 : 0;
            q[i] = (uint32_t)((qr + B) & 0xff) | ((uint32_t)((qg + B) & 0xff) << 8) | ((uint32_t)((qb + B) & 0xff) << 16);
            if (DRGB) {
                bc1a_diffuse(er, i, r - (float)qr * (1.0f / 31.0f));
                bc1a_diffuse(eg, i, g - (float)qg * (1.0f / 63.0f));
                bc1a_diffuse(eb, i, b - (float)qb * (1.0f / 31.0f));
            }
        }
    }

    // ---- OptimizeRGB
    const float fsteps = three ? 2.0f : 3.0f;
    const int32_t last = three ? 2 : 3;
    const float c1 = three ? 1.0f / 2.0f : 2.0f / 3.0f, c2 = three ? 0.0f / 2.0f : 1.0f / 3.0f;     // pC3 / pC4 [1], [2]; [0] = 1, pC4[3] = 0
    const float d1 = three ? 1.0f / 2.0f : 1.0f / 3.0f, d2 = three ? 2.0f / 2.0f : 2.0f / 3.0f;     // pD3 / pD4 [1], [2]; [0] = 0, pD4[3] = 1
    Rgb X = {lr, 1.0f, lb}, Y = {0.0f, 0.0f, 0.0f};
BC1A_UNROLL
    for (int i = 0; i < 16; i++) {
        const Rgb p = bc1a_point<DRGB>(q[i], lr, lb);
        if (p.r < X.r) X.r = p.r;
        if (p.g < X.g) X.g = p.g;
        if (p.b < X.b) X.b = p.b;
        if (p.r > Y.r) Y.r = p.r;
        if (p.g > Y.g) Y.g = p.g;
        if (p.b > Y.b) Y.b = p.b;
    }
    {
        const Rgb AB = {Y.r - X.r, Y.g - X.g, Y.b - X.b};
        const float fAB = AB.r * AB.r + AB.g * AB.g + AB.b * AB.b;
        if (!(fAB < FLT_MIN)) {                                    // else: a single colour, X and Y as they are
            const float inv = 1.0f / fAB;
            const Rgb D = {AB.r * inv, AB.g * inv, AB.b * inv};
            const Rgb M = {(X.r + Y.r) * 0.5f, (X.g + Y.g) * 0.5f, (X.b + Y.b) * 0.5f};
            float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f, f3 = 0.0f;
BC1A_UNROLL
            for (int i = 0; i < 16; i++) {
                const Rgb p = bc1a_point<DRGB>(q[i], lr, lb);
                const float pr = (p.r - M.r) * D.r, pg = (p.g - M.g) * D.g, pb = (p.b - M.b) * D.b;
                float f;
                f = pr + pg + pb; f0 += f * f;
                f = pr + pg - pb; f1 += f * f;
                f = pr - pg + pb; f2 += f * f;
                f = pr - pg - pb; f3 += f * f;
            }
            float fmax = f0;
            int imax = 0;
            if (f1 > fmax) { fmax = f1; imax = 1; }
            if (f2 > fmax) { fmax = f2; imax = 2; }
            if (f3 > fmax) { fmax = f3; imax = 3; }
            if (imax & 2) { const float f = X.g; X.g = Y.g; Y.g = f; }
            if (imax & 1) { const float f = X.b; X.b = Y.b; Y.b = f; }

            if (!(fAB < 1.0f / 4096.0f)) {                         // else: two colours
                constexpr float EPS = (0.25f / 64.0f) * (0.25f / 64.0f);
BC1A_NOUNROLL
                for (int it = 0; it < 8; it++) {
                    Rgb S0, S1, S2, S3;
                    S0.r = X.r * 1.0f + Y.r * 0.0f; S0.g = X.g * 1.0f + Y.g * 0.0f; S0.b = X.b * 1.0f + Y.b * 0.0f;
                    S1.r = X.r * c1 + Y.r * d1;     S1.g = X.g * c1 + Y.g * d1;     S1.b = X.b * c1 + Y.b * d1;
                    S2.r = X.r * c2 + Y.r * d2;     S2.g = X.g * c2 + Y.g * d2;     S2.b = X.b * c2 + Y.b * d2;
                    S3.r = X.r * 0.0f + Y.r * 1.0f; S3.g = X.g * 0.0f + Y.g * 1.0f; S3.b = X.b * 0.0f + Y.b * 1.0f;   // (four steps only)
                    Rgb Dir = {Y.r - X.r, Y.g - X.g, Y.b - X.b};
                    const float len = Dir.r * Dir.r + Dir.g * Dir.g + Dir.b * Dir.b;
                    if (len < 1.0f / 4096.0f) break;
                    const float scale = fsteps / len;
                    Dir.r *= scale; Dir.g *= scale; Dir.b *= scale;
                    float d2X = 0.0f, d2Y = 0.0f;
                    Rgb dX = {0.0f, 0.0f, 0.0f}, dY = {0.0f, 0.0f, 0.0f};
BC1A_UNROLL
                    for (int i = 0; i < 16; i++) {
                        const Rgb p = bc1a_point<DRGB>(q[i], lr, lb);
                        const float dot = (p.r - X.r) * Dir.r + (p.g - X.g) * Dir.g + (p.b - X.b) * Dir.b;
                        const int32_t k = (dot <= 0.0f) ? 0 : (dot >= fsteps) ? last : (int32_t)(dot + 0.5f);
                        const float pc = k == 0 ? 1.0f : k == 1 ? c1 : k == 2 ? c2 : 0.0f;
                        const float pd = k == 0 ? 0.0f : k == 1 ? d1 : k == 2 ? d2 : 1.0f;
                        Rgb diff;
                        diff.r = (k == 0 ? S0.r : k == 1 ? S1.r : k == 2 ? S2.r : S3.r) - p.r;
                        diff.g = (k == 0 ? S0.g : k == 1 ? S1.g : k == 2 ? S2.g : S3.g) - p.g;
                        diff.b = (k == 0 ? S0.b : k == 1 ? S1.b : k == 2 ? S2.b : S3.b) - p.b;
                        const float fc = pc * (1.0f / 8.0f), fd = pd * (1.0f / 8.0f);
                        d2X += fc * pc;
                        dX.r += fc * diff.r; dX.g += fc * diff.g; dX.b += fc * diff.b;
                        d2Y += fd * pd;
                        dY.r += fd * diff.r; dY.g += fd * diff.g; dY.b += fd * diff.b;
                    }
                    if (d2X > 0.0f) { const float f = -1.0f / d2X; X.r += dX.r * f; X.g += dX.g * f; X.b += dX.b * f; }
                    if (d2Y > 0.0f) { const float f = -1.0f / d2Y; Y.r += dY.r * f; Y.g += dY.g * f; Y.b += dY.b * f; }
                    if ((dX.r * dX.r < EPS) && (dX.g * dX.g < EPS) && (dX.b * dX.b < EPS) && (dY.r * dY.r < EPS) && (dY.g * dY.g < EPS) && (dY.b * dY.b < EPS))
                        break;                                     // (after the endpoints have moved)
                }
            }
        }
    }

    // ---- EncodeBC1, the endpoints
    Rgb C = {X.r * ir, X.g, X.b * ib}, D = {Y.r * ir, Y.g, Y.b * ib};
    const uint32_t wa = bc1a_encode565(C), wb = bc1a_encode565(D);
    if (!three && wa == wb) return bc1a_block(wa | (wb << 16), 0u);
    C = bc1a_decode565(wa);
    D = bc1a_decode565(wb);
    const Rgb A = {C.r * lr, C.g, C.b * lb}, Bc = {D.r * lr, D.g, D.b * lb};
    const bool ab = three == (wa <= wb);
    const uint32_t ends = ab ? (wa | (wb << 16)) : (wb | (wa << 16));
    const Rgb T0 = ab ? A : Bc, T1 = ab ? Bc : A;
    const Rgb T2 = bc1a_lerp(T0, T1, three ? 0.5f : 1.0f / 3.0f);
    const Rgb T3 = bc1a_lerp(T0, T1, 2.0f / 3.0f);                 // (four steps only)
    Rgb Dir = {T1.r - T0.r, T1.g - T0.g, T1.b - T0.b};
    const float scale = (wa != wb) ? (fsteps / (Dir.r * Dir.r + Dir.g * Dir.g + Dir.b * Dir.b)) : 0.0f;
    Dir.r *= scale; Dir.g *= scale; Dir.b *= scale;

    // ---- EncodeBC1, the indices (error diffusion of the chosen steps with DITHER_RGB; a transparent texel diffuses nothing)
    uint32_t dw = 0;
    float er[16], eg[16], eb[16];
    if (DRGB) {
BC1A_UNROLL
        for (int i = 0; i < 16; i++) er[i] = eg[i] = eb[i] = 0.0f;
    }
BC1A_UNROLL
    for (int i = 0; i < 16; i++) {
        if (three && ((key >> i) & 1u)) {
            dw = (3u << 30) | (dw >> 2);
        } else {
            float r = (float)(w[i] & 0xffu) * BC1A_UNORM * lr, g = (float)((w[i] >> 8) & 0xffu) * BC1A_UNORM, b = (float)((w[i] >> 16) & 0xffu) * BC1A_UNORM * lb;
            if (DRGB) { r += er[i]; g += eg[i]; b += eb[i]; }
            const float dot = (r - T0.r) * Dir.r + (g - T0.g) * Dir.g + (b - T0.b) * Dir.b;
            uint32_t step;                                         // pSteps3 = {0, 2, 1}, pSteps4 = {0, 2, 3, 1}
            if (dot <= 0.0f) step = 0;
            else if (dot >= fsteps) step = 1;
            else { const int32_t k = (int32_t)(dot + 0.5f); step = k == 0 ? 0u : k == 1 ? 2u : (k == 2 && !three) ? 3u : 1u; }
            dw = (step << 30) | (dw >> 2);
            if (DRGB) {
                bc1a_diffuse(er, i, r - (step == 0 ? T0.r : step == 1 ? T1.r : step == 2 ? T2.r : T3.r));
                bc1a_diffuse(eg, i, g - (step == 0 ? T0.g : step == 1 ? T1.g : step == 2 ? T2.g : T3.g));
                bc1a_diffuse(eb, i, b - (step == 0 ? T0.b : step == 1 ? T1.b : step == 2 ? T2.b : T3.b));
            }
        }
    }
    return bc1a_block(ends, dw);
}

} // namespace bc1a
} // namespace itw
