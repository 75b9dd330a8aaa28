// bc2_core.hpp -- the arithmetic of the BC2 encoder: DirectXTex's D3DXEncodeBC2 (BC.cpp:820-890; COLOR_WEIGHTS is not defined there, BC.cpp:19),
// restated for one block in registers.  The alpha half is here; the colour half is EncodeBC1(..., bColorKey = false, 0.f, flags), which is what
// bc1a_core.hpp's bc1a_encode computes for alpha_ref = 0.0f without its DITHER_A bit: no texel's alpha is below 0, so uSteps == 4 and the
// 3-step test never fires, and EncodeBC1 never reads BC_FLAGS_DITHER_A.  Plain C++ under bc1a_core.hpp's macros, so the same text is the
// kernel's (bc2.hip) and a host program's (tools/bc2_host_check.cpp).  fp32 throughout, one rounding per operation: -ffp-contract=off.
#pragma once
#include <cstdint>
#include "bc1a_core.hpp"

namespace itw {
namespace bc2 {

struct Bc2Block { uint32_t alpha0, alpha1, ends, bitmap; };      // bitmap[0], bitmap[1] (texel i in nibble i & 7 of word i >> 3), then the BC1 block

// The 4-bit alpha half (BC.cpp:834-878).  The word is built as the source builds it: `>>= 4; |= u << 28` in 32 bits.  A u above 15 would
// spill into the nibbles of the texels before it, as the source's does, and the expression is kept so that it would.  Without dithering
// fAlph <= 1.0f (255 * fl(1/255) rounds to 1.0f), so u <= 15.  With it a texel's error is a combination (weights 7/16, 3/16, 5/16, 1/16: at
// most 1 in sum) of its neighbours' differences, each in [-1/30, 1/30) in real arithmetic, so fAlph * 15 + 0.5 stays below 16 there; what
// fp32 rounding leaves of that margin is discussed in DESIGN.md 3.15 (tests/_dxtex_bc2.py's model counts the texels with u > 15).  The cast
// truncates toward zero.
template <bool DITHER_A>
BC1A_FN void bc2_alpha(const uint32_t (&w)[16], uint32_t& a0, uint32_t& a1)
{
    uint32_t bm[2] = {0u, 0u};
    float e[16];
    if (DITHER_A) {
BC1A_UNROLL
        for (int i = 0; i < 16; i++) e[i] = 0.0f;
    }
BC1A_UNROLL
    for (int i = 0; i < 16; i++) {
        float alph = (float)(w[i] >> 24) * bc1a::BC1A_UNORM;
        if (DITHER_A) alph += e[i];
        const uint32_t u = (uint32_t)(int32_t)(alph * 15.0f + 0.5f);
        bm[i >> 3] >>= 4;
        bm[i >> 3] |= u << 28;
        if (DITHER_A) bc1a::bc1a_diffuse(e, i, alph - (float)u * (1.0f / 15.0f));
    }
    a0 = bm[0];
    a1 = bm[1];
}

// One block: w = its sixteen RGBA8 texels (R in the low byte), raster order.  DITHER: bc1a's template bits (BC1A_DITHER_RGB, BC1A_DITHER_A).
// The alpha pass runs first and leaves only its two words, so its error array is dead before OptimizeRGB starts.
template <uint32_t DITHER>
BC1A_FN Bc2Block bc2_encode(const uint32_t (&w)[16], bool uniform)
{
    Bc2Block o;
    bc2_alpha<(DITHER & bc1a::BC1A_DITHER_A) != 0>(w, o.alpha0, o.alpha1);
    const bc1a::Bc1aBlock c = bc1a::bc1a_encode<(DITHER & bc1a::BC1A_DITHER_RGB)>(w, 0.0f, uniform);
    o.ends = c.ends;
    o.bitmap = c.bitmap;
    return o;
}

} // namespace bc2
} // namespace itw
