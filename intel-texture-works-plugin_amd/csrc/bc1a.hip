// bc1a.hip -- BC1 with 1-bit alpha (punch-through, "DXT1A") for gfx950 (MI355X): DirectXTex's colour-key encoder.
//
// Restates D3DXEncodeBC1 -> EncodeBC1(bColorKey = true) -> OptimizeRGB (DirectXTex BC.cpp:67-318, 372-677, 729-787; COLOR_WEIGHTS is not
// defined there) byte for byte: plain fp32, one rounding per operation (the library is built with -ffp-contract=off, unflushed denormals
// and correctly rounded divides), every sum over a block's texels in the source's order 0..15.
//
// Mapping: ONE LANE PER BLOCK.  Every sum of the source (fDir[4], d2X / d2Y / dX / dY, the error diffusion) runs over texels 0..15 in
// order; a split across lanes would re-associate it.  A lane loads its four 16-byte rows (contiguous with its
// neighbours'), keeps the sixteen packed RGBA8 words and the sixteen quantised 5:6:5 points as packed integers (the dithered ones biased
// by 4 so that they stay unsigned bytes) and converts on use: the conversions are deterministic, and 32 registers replace 112 floats.
// Every loop over texels and steps is fully unrolled, so the error arrays and the diffusion targets (i + 1, i + 3, i + 4, i + 5) have
// compile-time indices, and pSteps[iStep] / pC[iStep] / pD[iStep] / Step[iStep] / pSteps3 / pSteps4 are selects: no scratch.  Only the
// Newton iterations stay a loop (nothing is indexed by the iteration).  The kernel is a template on the two dither bits, so the plain
// variant carries neither error array; BC_FLAGS_UNIFORM is a uniform runtime value: it turns the luminance weights into 1.0f, and a
// multiplication by 1.0f is the identity in IEEE arithmetic (the source skips the multiplication instead).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/itw_dispatch.h"
#include "bc1a_core.hpp"
#include "host_rt.hpp"
#include "kernels.hpp"

namespace itw {

// One lane per block, 64 blocks per wave.  VEC16: src and stride are 16-byte aligned (a row of a block is one 16-byte load); otherwise
// four dword loads.  Partial blocks (width or height no multiple of 4) are filled by DirectXTex's {0, 0, 0, 1} rule (bc45_fill_index).
template <uint32_t DITHER, bool VEC16>
__global__ void __launch_bounds__(256)
bc1a_kernel(const uint8_t* __restrict__ src, int64_t stride, int32_t width, int32_t height, int32_t blocks_x, int32_t nblocks,
            uint8_t* __restrict__ dst, float alpha_ref, int32_t uniform)
{
    const int32_t b = (int32_t)(blockIdx.x * 256u + threadIdx.x);
    if (b >= nblocks) return;
    const int32_t yy = b / blocks_x, xx = b - yy * blocks_x;
    const int32_t pw = min(4, width - 4 * xx), ph = min(4, height - 4 * yy);
    const uint8_t* p = src + (int64_t)yy * 4 * stride + (int64_t)xx * 16;
    uint32_t w[16];
    if (pw == 4 && ph == 4) {
#pragma unroll
        for (int y = 0; y < 4; y++) {
            const uint8_t* row = p + (int64_t)y * stride;
            if (VEC16) {
                const uint4 v = *reinterpret_cast<const uint4*>(row);
                w[4 * y] = v.x; w[4 * y + 1] = v.y; w[4 * y + 2] = v.z; w[4 * y + 3] = v.w;
            } else {
                const uint32_t* t = reinterpret_cast<const uint32_t*>(row);
                w[4 * y] = t[0]; w[4 * y + 1] = t[1]; w[4 * y + 2] = t[2]; w[4 * y + 3] = t[3];
            }
        }
    } else {
#pragma unroll
        for (int y = 0; y < 4; y++) {
            const uint8_t* row = p + (int64_t)bc45_fill_index(y, ph) * stride;
#pragma unroll
            for (int x = 0; x < 4; x++) w[4 * y + x] = reinterpret_cast<const uint32_t*>(row)[bc45_fill_index(x, pw)];
        }
    }
    const bc1a::Bc1aBlock o = bc1a::bc1a_encode<DITHER>(w, alpha_ref, uniform != 0);
    *reinterpret_cast<uint2*>(dst + (int64_t)b * 8) = make_uint2(o.ends, o.bitmap);
}

template <uint32_t DITHER>
static void launch_bc1a_variant(const uint8_t* src, int64_t stride, int width, int height, int bx, int32_t n, uint8_t* dst, float alpha_ref, int32_t uniform, hipStream_t st)
{
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride) & 15) == 0;
    const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
    if (vec) hipLaunchKernelGGL((bc1a_kernel<DITHER, true>),  grid, blk, 0, st, src, stride, width, height, bx, n, dst, alpha_ref, uniform);
    else     hipLaunchKernelGGL((bc1a_kernel<DITHER, false>), grid, blk, 0, st, src, stride, width, height, bx, n, dst, alpha_ref, uniform);
}

void launch_bc1a(const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, float alpha_ref, uint32_t flags, hipStream_t st)
{
    if (width <= 0 || height <= 0) return;
    const int bx = (width + 3) / 4, by = (height + 3) / 4;        // DirectXTex keeps partial blocks
    const int64_t n = (int64_t)bx * by;
    if (n > (int64_t)INT32_MAX - 255) fail_msg("BC1A: %d x %d is more blocks than one launch covers", width, height);
    if ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride) & 3) fail_msg("BC1A: texels and stride must be 4-byte aligned");
    const int32_t uniform = (flags & ITW_BC_UNIFORM) ? 1 : 0;
    switch (((flags & ITW_BC_DITHER_RGB) ? bc1a::BC1A_DITHER_RGB : 0u) | ((flags & ITW_BC_DITHER_A) ? bc1a::BC1A_DITHER_A : 0u)) {
    case 0:  launch_bc1a_variant<0>(src, stride, width, height, bx, (int32_t)n, dst, alpha_ref, uniform, st); break;
    case 1:  launch_bc1a_variant<1>(src, stride, width, height, bx, (int32_t)n, dst, alpha_ref, uniform, st); break;
    case 2:  launch_bc1a_variant<2>(src, stride, width, height, bx, (int32_t)n, dst, alpha_ref, uniform, st); break;
    default: launch_bc1a_variant<3>(src, stride, width, height, bx, (int32_t)n, dst, alpha_ref, uniform, st); break;
    }
}

} // namespace itw
