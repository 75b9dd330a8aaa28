// bc3_dxtex.hip -- BC3 (DXT4 / DXT5) by DirectXTex's encoder for gfx950 (MI355X): D3DXEncodeBC3, beside kernel.ispc's CompressBlocksBC3 (bc1_bc3.hip),
// which stays the encoder of DXGI 77 / 78.  The two codes ITW_FORMAT_BC3_DXTEX[_SRGB] (itw_dispatch.h) reach this file.
//
// Restates D3DXEncodeBC3 (DirectXTex BC.cpp:939-1139; COLOR_WEIGHTS is not defined there) byte for byte.  The alpha half is bc3_core.hpp's
// bc3_alpha; the colour half is EncodeBC1(bColorKey = false, 0.f, flags), which bc1a_core.hpp's bc1a_encode computes for alpha_ref = 0.0f
// without its DITHER_A bit (bc2_core.hpp says why).  Plain fp32, one rounding per operation (-ffp-contract=off).
//
// Mapping: ONE LANE PER BLOCK, as bc1a.hip and bc2.hip and for their reason: every sum of the source runs over texels 0..15 in order, and a
// split across lanes would re-associate it.  A lane loads its four 16-byte rows (contiguous with its neighbours'), runs the alpha pass first
// and keeps only its two words -- the points, the error arrays and the step tables are dead before OptimizeRGB starts, so the colour half has
// bc1a's register budget -- and stores its block with one 16-byte store: .x / .y the alpha half, .z the endpoints, .w the indices.  Every
// loop over texels is fully unrolled, so the error arrays and the diffusion targets have compile-time indices, and a value picked by a step
// known only at run time comes through selects (bc3_pick): no scratch.  A template on the two dither bits; BC_FLAGS_UNIFORM is a uniform
// runtime value, as in bc1a.hip.  The early outs of the alpha half (all opaque; 8 steps with equal endpoints) are per lane.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/itw_dispatch.h"
#include "bc3_core.hpp"
#include "host_rt.hpp"
#include "kernels.hpp"

namespace itw {

// One lane per block, 64 blocks per wave.  VEC16: src and stride are 16-byte aligned (a row of a block is one 16-byte load); otherwise
// four dword loads.  Partial blocks (width or height no multiple of 4) are filled by DirectXTex's {0, 0, 0, 1} rule (bc45_fill_index).
// dst16 (uniform): dst is 16-byte aligned and the block goes out in one store; otherwise (a target inside a file's payload) four dwords.
template <uint32_t DITHER, bool VEC16>
__global__ void __launch_bounds__(256)
bc3_dxtex_kernel(const uint8_t* __restrict__ src, int64_t stride, int32_t width, int32_t height, int32_t blocks_x, int32_t nblocks,
                 uint8_t* __restrict__ dst, int32_t uniform, int32_t dst16)
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
    const bc3::Bc3Block o = bc3::bc3_encode<DITHER>(w, uniform != 0);
    uint8_t* q = dst + (int64_t)b * 16;
    if (dst16) {
        *reinterpret_cast<uint4*>(q) = make_uint4(o.alpha0, o.alpha1, o.ends, o.bitmap);
    } else {
        uint32_t* t = reinterpret_cast<uint32_t*>(q);
        t[0] = o.alpha0; t[1] = o.alpha1; t[2] = o.ends; t[3] = o.bitmap;
    }
}

template <uint32_t DITHER>
static void launch_bc3_dxtex_variant(const uint8_t* src, int64_t stride, int width, int height, int bx, int32_t n, uint8_t* dst, int32_t uniform, hipStream_t st)
{
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride) & 15) == 0;
    const int32_t dst16 = (reinterpret_cast<uintptr_t>(dst) & 15) == 0 ? 1 : 0;
    const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
    if (vec) hipLaunchKernelGGL((bc3_dxtex_kernel<DITHER, true>),  grid, blk, 0, st, src, stride, width, height, bx, n, dst, uniform, dst16);
    else     hipLaunchKernelGGL((bc3_dxtex_kernel<DITHER, false>), grid, blk, 0, st, src, stride, width, height, bx, n, dst, uniform, dst16);
}

void launch_bc3_dxtex(const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, uint32_t flags, hipStream_t st)
{
    if (width <= 0 || height <= 0) return;
    const int bx = (width + 3) / 4, by = (height + 3) / 4;        // DirectXTex keeps partial blocks
    const int64_t n = (int64_t)bx * by;
    if (n > (int64_t)INT32_MAX - 255) fail_msg("BC3 (DirectXTex): %d x %d is more blocks than one launch covers", width, height);
    if ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride) & 3) fail_msg("BC3 (DirectXTex): texels and stride must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(dst) & 3) fail_msg("BC3 (DirectXTex): the target must be 4-byte aligned");
    const int32_t uniform = (flags & ITW_BC_UNIFORM) ? 1 : 0;
    switch (((flags & ITW_BC_DITHER_RGB) ? bc1a::BC1A_DITHER_RGB : 0u) | ((flags & ITW_BC_DITHER_A) ? bc1a::BC1A_DITHER_A : 0u)) {
    case 0:  launch_bc3_dxtex_variant<0>(src, stride, width, height, bx, (int32_t)n, dst, uniform, st); break;
    case 1:  launch_bc3_dxtex_variant<1>(src, stride, width, height, bx, (int32_t)n, dst, uniform, st); break;
    case 2:  launch_bc3_dxtex_variant<2>(src, stride, width, height, bx, (int32_t)n, dst, uniform, st); break;
    default: launch_bc3_dxtex_variant<3>(src, stride, width, height, bx, (int32_t)n, dst, uniform, st); break;
    }
}

} // namespace itw
