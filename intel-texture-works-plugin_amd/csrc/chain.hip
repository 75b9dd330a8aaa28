// chain.hip -- the gather step of a whole mip chain / cube map encode (include/itw_dispatch.h: itwCompressImageChain).
//
// The encoders take one surface.  A chain is many small, unpadded images: level 0 .. n of every face, in DDS order.  Their blocks are
// independent, so a GROUP of consecutive images becomes ONE packed surface -- P blocks wide, ceil(n / P) block rows high, packed block j
// = block j of the group's concatenated block list -- and the encoders' raster-order output of the first n packed blocks is exactly the
// group's slice of the DDS payload (abi.hip, compress_chain).  This kernel builds that packed surface, applying each format's edge rule to
// images whose size is not a multiple of 4: edge replication for BC1/BC3/BC6H/BC7 (the plugin's DoPaddingToMultiplesOf4,
// itwPadToMultipleOf4), DirectXTex's partial-block fill for BC4/BC5 (bc45_fill_index, the rule of the BC4/BC5 kernel's own load).
//
// Memory only: one lane per 4-texel block row (16 B of RGBA8, 32 B of RGBA16F), 64 blocks per workgroup with wave r carrying texel row r,
// so a wave reads 64 consecutive blocks of one image row -- adjacent in the source -- and writes 64 adjacent 16/32-B pieces of one packed row.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.hpp"
#include "host_rt.hpp"
#include "normal_prep.hpp"

namespace {
using itw::ChainImage;
using itw::bc45_fill_index;

// a texel's first dword from a source whose alignment is whatever the caller's pointer and stride make it
__device__ __forceinline__ uint32_t load_u32(const uint8_t* p)
{
    if (((uintptr_t)p & 3) == 0) return *reinterpret_cast<const uint32_t*>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// PX: bytes per texel (4 RGBA8, 8 RGBA16F).  FILL45: BC4/BC5's partial-block fill instead of edge replication.  EXTENTS: the lane that
// carries texel row 0 of block j < nblocks also writes extents[j] = (pw - 1) | (ph - 1) << 2, the part of the block that lies inside its
// image (itwCompressImageChainRefined leaves the padding out of a block's error).  OPS (trailing, so that the instantiations without it
// stay what they were): the normal-map stages of normal_prep.hpp applied to every texel copied (itwCompressNormalMapChain); a replicated
// texel is prepared like the one it repeats, so the packed surface is the gather of prepared images.
// SRC (trailing likewise; PX 4 and FILL45 only): the images are signed normal sources of SRC-byte texels (4 RGBA8_SNORM, 8 RGBA16F, 16 RGBA32F;
// itwCompressSignedNormalMapChain) and OPS has its signed meaning: every texel is loaded, flipped / normalised in fp32 and quantised to its
// RGBA8_SNORM word as it is copied (normal_prep.hpp), so the packed surface is the gather of images quantised by itwQuantizeNormalMapChain.
template <int PX, bool FILL45, bool EXTENTS, uint32_t OPS = 0, int SRC = 0>
__global__ void __launch_bounds__(256) chain_gather_kernel(const ChainImage* __restrict__ images, int32_t nimg, int64_t nblocks,
                                                          int32_t packed_bx, int64_t total, uint8_t* __restrict__ dst, int64_t dst_pitch,
                                                          uint8_t* __restrict__ extents)
{
    constexpr int W = PX;                                       // dwords per 4-texel row piece (4 or 8)
    constexpr int SPX = SRC ? SRC : PX;                         // bytes per SOURCE texel = dwords per 4-texel piece of a source row
    static_assert(SRC == 0 || (PX == 4 && FILL45 && !EXTENTS), "a signed normal source is gathered for BC4_SNORM / BC5_SNORM");
    const int r = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    if (j >= total) return;
    const int64_t prow = j / packed_bx, pcol = j - prow * packed_bx;
    uint4* out = reinterpret_cast<uint4*>(dst + (prow * 4 + r) * dst_pitch + pcol * 4 * PX);
    uint32_t v[W];
    if (j >= nblocks) {                                         // tail of the last packed row: encoded into scratch and dropped
#pragma unroll
        for (int q = 0; q < W; q++) v[q] = 0u;
    } else {
        int lo = 0, hi = nimg - 1;                              // the last image whose first block is <= j
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (images[mid].first_block <= j) lo = mid; else hi = mid - 1;
        }
        const ChainImage im = images[lo];
        const int32_t bw = (im.width + 3) >> 2;
        const int64_t b = j - im.first_block;
        const int32_t by = (int32_t)(b / bw), bx = (int32_t)(b - (int64_t)by * bw);
        const int32_t x0 = bx * 4, y0 = by * 4;
        const int32_t pw = min(4, im.width - x0), ph = min(4, im.height - y0);
        if (EXTENTS && r == 0) extents[j] = (uint8_t)((pw - 1) | ((ph - 1) << 2));
        const int32_t y = y0 + (FILL45 ? bc45_fill_index(r, ph) : min(r, ph - 1));
        const uint8_t* p = im.ptr + (int64_t)y * im.stride + (int64_t)x0 * SPX;
        uint32_t s[SPX];                                        // the four source texels (without SRC they are the output: copied below)
        if (pw == 4 && ((uintptr_t)p & 15) == 0) {
#pragma unroll
            for (int q = 0; q < SPX / 4; q++) {
                const uint4 t = reinterpret_cast<const uint4*>(p)[q];
                s[4 * q] = t.x; s[4 * q + 1] = t.y; s[4 * q + 2] = t.z; s[4 * q + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int sx = FILL45 ? bc45_fill_index(c, pw) : min(c, pw - 1);
#pragma unroll
                for (int q = 0; q < SPX / 4; q++) s[c * (SPX / 4) + q] = load_u32(p + sx * SPX + q * 4);
            }
        }
        if (SRC != 0) {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                float f[4];
                itw::normal_load_signed<SRC ? SRC : 4>(f, &s[c * (SPX / 4)]);
                v[c] = itw::normal_quantize_texel(f, OPS);
            }
        } else {
#pragma unroll
            for (int q = 0; q < W; q++) v[q] = s[q];
        }
        if (SRC == 0 && OPS != 0) {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                if (PX == 4) v[c] = itw::normal_prep_rgba8(v[c], OPS);
                else itw::normal_prep_rgba16f(v[2 * c], v[2 * c + 1], OPS);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < W / 4; q++) out[q] = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}

// the gather with the normal-map stages: OPS is a template argument, so one instantiation per value of the bit set
template <int PX, bool FILL45, uint32_t OPS>
void launch_prepared(uint32_t ops, dim3 grid, hipStream_t st, const ChainImage* images, int32_t nimg, int64_t nblocks, int32_t packed_bx, int64_t total,
                     uint8_t* dst, int64_t dst_pitch)
{
    if constexpr (OPS > itw::NORMAL_OPS_ALL) itw::fail_msg("launch_chain_gather: normal-map ops %u", ops);
    else if (ops == OPS)
        hipLaunchKernelGGL((chain_gather_kernel<PX, FILL45, false, OPS>), grid, dim3(256), 0, st, images, nimg, nblocks, packed_bx, total, dst, dst_pitch,
                           (uint8_t*)nullptr);
    else launch_prepared<PX, FILL45, OPS + 1>(ops, grid, st, images, nimg, nblocks, packed_bx, total, dst, dst_pitch);
}

// the gather of signed normal sources: SRC and OPS are template arguments, one instantiation per (texel kind, bit set)
template <int SRC, uint32_t OPS>
void launch_signed(uint32_t ops, dim3 grid, hipStream_t st, const ChainImage* images, int32_t nimg, int64_t nblocks, int32_t packed_bx, int64_t total,
                   uint8_t* dst, int64_t dst_pitch)
{
    if constexpr (OPS > itw::NORMAL_OPS_ALL) itw::fail_msg("launch_chain_gather: normal-map ops %u", ops);
    else if (ops == OPS)
        hipLaunchKernelGGL((chain_gather_kernel<4, true, false, OPS, SRC>), grid, dim3(256), 0, st, images, nimg, nblocks, packed_bx, total, dst, dst_pitch,
                           (uint8_t*)nullptr);
    else launch_signed<SRC, OPS + 1>(ops, grid, st, images, nimg, nblocks, packed_bx, total, dst, dst_pitch);
}

} // namespace

namespace itw {

void launch_chain_gather(const ChainImage* images, int nimg, int64_t nblocks, int packed_bx, int packed_by, int texel_bytes, bool fill45,
                         uint8_t* dst, int64_t dst_pitch, hipStream_t st, uint8_t* extents, uint32_t normal_ops, int signed_source)
{
    const int64_t total = (int64_t)packed_bx * packed_by;
    if (total <= 0 || nimg <= 0) return;
    if (nblocks > total || (dst_pitch & 15) || ((uintptr_t)dst & 15) || dst_pitch < (int64_t)packed_bx * 4 * texel_bytes)
        fail_msg("launch_chain_gather: %lld blocks into %d x %d packed blocks, pitch %lld", (long long)nblocks, packed_bx, packed_by, (long long)dst_pitch);
    const dim3 grid((unsigned)((total + 63) / 64)), blk(256);
    if (signed_source != 0) {
        if (extents || texel_bytes != 4 || !fill45) fail_msg("launch_chain_gather: a signed normal source is gathered into an RGBA8_SNORM surface for BC4 / BC5");
        if (signed_source == 4)       launch_signed<4, 0>(normal_ops, grid, st, images, nimg, nblocks, packed_bx, total, dst, dst_pitch);
        else if (signed_source == 8)  launch_signed<8, 0>(normal_ops, grid, st, images, nimg, nblocks, packed_bx, total, dst, dst_pitch);
        else if (signed_source == 16) launch_signed<16, 0>(normal_ops, grid, st, images, nimg, nblocks, packed_bx, total, dst, dst_pitch);
        else fail_msg("launch_chain_gather: signed source texels of %d bytes", signed_source);
        ITW_CHECK(hipGetLastError());
        return;
    }
    if (normal_ops != 0) {
        if (extents) fail_msg("launch_chain_gather: extents do not go with the normal-map stages");
        if (texel_bytes == 8 && fill45) fail_msg("launch_chain_gather: the BC4/BC5 fill is for RGBA8 surfaces");
        if (texel_bytes == 8) launch_prepared<8, false, 1>(normal_ops, grid, st, images, nimg, nblocks, packed_bx, total, dst, dst_pitch);
        else if (fill45)      launch_prepared<4, true, 1>(normal_ops, grid, st, images, nimg, nblocks, packed_bx, total, dst, dst_pitch);
        else                  launch_prepared<4, false, 1>(normal_ops, grid, st, images, nimg, nblocks, packed_bx, total, dst, dst_pitch);
        ITW_CHECK(hipGetLastError());
        return;
    }
    if (texel_bytes == 8) {
        if (fill45) fail_msg("launch_chain_gather: the BC4/BC5 fill is for RGBA8 surfaces");
        if (extents) hipLaunchKernelGGL((chain_gather_kernel<8, false, true>), grid, blk, 0, st, images, nimg, nblocks, packed_bx, total, dst, dst_pitch, extents);
        else         hipLaunchKernelGGL((chain_gather_kernel<8, false, false>), grid, blk, 0, st, images, nimg, nblocks, packed_bx, total, dst, dst_pitch, extents);
    } else if (fill45) {
        if (extents) fail_msg("launch_chain_gather: extents go with edge replication");
        hipLaunchKernelGGL((chain_gather_kernel<4, true, false>), grid, blk, 0, st, images, nimg, nblocks, packed_bx, total, dst, dst_pitch, extents);
    } else {
        if (extents) hipLaunchKernelGGL((chain_gather_kernel<4, false, true>), grid, blk, 0, st, images, nimg, nblocks, packed_bx, total, dst, dst_pitch, extents);
        else         hipLaunchKernelGGL((chain_gather_kernel<4, false, false>), grid, blk, 0, st, images, nimg, nblocks, packed_bx, total, dst, dst_pitch, extents);
    }
    ITW_CHECK(hipGetLastError());
}

} // namespace itw
