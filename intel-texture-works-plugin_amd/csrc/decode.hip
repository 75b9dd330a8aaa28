// decode.hip -- BCn block decoders for gfx950 (include/itw_decode.h).  One block per lane: 8 / 16 B in, 64 B (RGBA8)
// or 128 B (RGBA16F) out as four row stores of 16 / 32 B per lane.  Pure integer work, HBM bound by the output
// (4-8x the input).  Written from the format definitions (the readable statement inside the reference tree is its
// decoder: BC.cpp for BC1/BC3, BC6HBC7.cpp:35-37 weights, :40 partitions, :247 fix-ups, :537 BC7 mode table,
// :1937-2140 BC7 decode, :310-500 BC6H mode descriptors, :1077-1210 BC6H decode, :1313-1359 unquantisation).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include "../../include/itw_decode.h"
#include "../../include/itw_amd.h"
#include "decode_core.hpp"
#include "host_rt.hpp"

namespace itw {

// FMT: 1 BC1, 3 BC3, 4 BC4, 5 BC5, 14 BC4_SNORM, 15 BC5_SNORM, 7 BC7, 6 BC6H
template <int FMT>
__global__ void __launch_bounds__(256)
decode_kernel(const uint8_t* __restrict__ blocks, int32_t blocks_x, int32_t nblocks, uint8_t* __restrict__ out, int64_t stride,
              int32_t* __restrict__ modes, int32_t width, int32_t height)
{
    const int32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nblocks) return;
    const int32_t yy = b / blocks_x, xx = b - yy * blocks_x;
    int mode = 0;
    if (FMT == 6) {
        const uint4 w = *reinterpret_cast<const uint4*>(blocks + (int64_t)b * 16);
        Bits bs{(unsigned long long)w.x | ((unsigned long long)w.y << 32), (unsigned long long)w.z | ((unsigned long long)w.w << 32), 0};
        uint32_t lo[16], hi[16];
        mode = decode_bc6h(bs, lo, hi);
        uint8_t* o = out + (int64_t)yy * 4 * stride + (int64_t)xx * 32;
#pragma unroll
        for (int y = 0; y < 4; y++) {
            uint32_t* row = reinterpret_cast<uint32_t*>(o + y * stride);
#pragma unroll
            for (int x = 0; x < 4; x++) { row[2 * x] = lo[y * 4 + x]; row[2 * x + 1] = hi[y * 4 + x]; }
        }
    } else {
        uint32_t px[16];
        if (FMT == 1) {
            const uint2 w = *reinterpret_cast<const uint2*>(blocks + (int64_t)b * 8);
            decode_color(w.x, w.y, true, px);
        } else if (FMT == 3) {
            const uint4 w = *reinterpret_cast<const uint4*>(blocks + (int64_t)b * 16);
            decode_color(w.z, w.w, false, px);
            decode_bc3_alpha(w.x, w.y, px);
        } else if (FMT == 4) {                                   // BC4_UNORM -> (R, 0, 0, 255) like D3DXDecodeBC4U (BC4BC5.cpp:373-385)
            const uint2 w = *reinterpret_cast<const uint2*>(blocks + (int64_t)b * 8);
#pragma unroll
            for (int k = 0; k < 16; k++) px[k] = 0xff000000u;
            decode_scalar_block<0>(w.x, w.y, px);
        } else if (FMT == 5) {                                   // BC5_UNORM -> (R, G, 0, 255) (BC4BC5.cpp:449-462)
            const uint4 w = *reinterpret_cast<const uint4*>(blocks + (int64_t)b * 16);
#pragma unroll
            for (int k = 0; k < 16; k++) px[k] = 0xff000000u;
            decode_scalar_block<0>(w.x, w.y, px);
            decode_scalar_block<8>(w.z, w.w, px);
        } else if (FMT == 14) {                                  // BC4_SNORM -> int8 (R, 0, 0, 127) like D3DXDecodeBC4S (BC4BC5.cpp:388-400)
            const uint2 w = *reinterpret_cast<const uint2*>(blocks + (int64_t)b * 8);
#pragma unroll
            for (int k = 0; k < 16; k++) px[k] = 0x7f000000u;
            decode_scalar_block_snorm<0>(w.x, w.y, px);
        } else if (FMT == 15) {                                  // BC5_SNORM -> int8 (R, G, 0, 127) (BC4BC5.cpp:465-478)
            const uint4 w = *reinterpret_cast<const uint4*>(blocks + (int64_t)b * 16);
#pragma unroll
            for (int k = 0; k < 16; k++) px[k] = 0x7f000000u;
            decode_scalar_block_snorm<0>(w.x, w.y, px);
            decode_scalar_block_snorm<8>(w.z, w.w, px);
        } else {
            const uint4 w = *reinterpret_cast<const uint4*>(blocks + (int64_t)b * 16);
            Bits bs{(unsigned long long)w.x | ((unsigned long long)w.y << 32), (unsigned long long)w.z | ((unsigned long long)w.w << 32), 0};
            mode = decode_bc7(bs, px);
        }
        uint8_t* o = out + (int64_t)yy * 4 * stride + (int64_t)xx * 16;
        // BC4 / BC5 streams may end in partial blocks (the encoder keeps them, itw_bc45.h): texels beyond the surface are cropped
        constexpr bool PARTIAL = FMT == 4 || FMT == 5 || FMT == 14 || FMT == 15;
        const int ny = PARTIAL ? min(4, height - yy * 4) : 4, nx = PARTIAL ? min(4, width - xx * 4) : 4;
#pragma unroll
        for (int y = 0; y < 4; y++) {
            if (y >= ny) break;
            uint32_t* row = reinterpret_cast<uint32_t*>(o + y * stride);
#pragma unroll
            for (int x = 0; x < 4; x++) if (x < nx) row[x] = px[y * 4 + x];
        }
    }
    if (modes) modes[b] = mode;
}

} // namespace itw

namespace {

bool on_device(const void* p) { return itw::is_device_pointer(p); }     // device and managed memory alike

#define DEC_CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "itwDecodeBlocks: %s failed: %s; aborting\n", #x, hipGetErrorString(e_)); std::abort(); } } while (0)

} // namespace

extern "C" int itwDecodeBlocks(int f, const uint8_t* blocks, int width, int height, uint8_t* out, int64_t out_stride, int32_t* modes)
{
    const int kind = (f == 71 || f == 72) ? 1 : (f == 77 || f == 78) ? 3 : (f == 98 || f == 99) ? 7 : (f == 95 || f == 96) ? 6 : f == 80 ? 4 : f == 83 ? 5 : f == 81 ? 14 : f == 84 ? 15 : 0;
    const bool partial_ok = (kind == 4 || kind == 5 || kind == 14 || kind == 15);   // the DirectXTex formats keep partial blocks
    if (!kind || (out_stride & 3)) return -1;
    if (partial_ok ? (width < 1 || height < 1) : (width < 4 || height < 4 || (width & 3) || (height & 3))) return -1;
    const int bx = (width + 3) / 4, by = (height + 3) / 4;
    const int64_t n = (int64_t)bx * by;
    const size_t in_bytes = (size_t)n * ((kind == 1 || kind == 4 || kind == 14) ? 8 : 16), texel = kind == 6 ? 8 : 4;
    const size_t row_bytes = (size_t)width * texel;
    if ((size_t)out_stride < row_bytes) return -1;
    hipStream_t st = (hipStream_t)itwGetStream();
    const bool din = on_device(blocks), dout = on_device(out), dmodes = !modes || on_device(modes);

    uint8_t *d_in = const_cast<uint8_t*>(blocks), *d_out = out;
    int32_t* d_modes = modes;
    int64_t d_stride = out_stride;
    if (!din)  { DEC_CHECK(hipMalloc((void**)&d_in, in_bytes)); DEC_CHECK(hipMemcpyAsync(d_in, blocks, in_bytes, hipMemcpyHostToDevice, st)); }
    if (!dout) { d_stride = (int64_t)row_bytes; DEC_CHECK(hipMalloc((void**)&d_out, row_bytes * (size_t)height)); }
    if (modes && !dmodes) DEC_CHECK(hipMalloc((void**)&d_modes, (size_t)n * 4));
    const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
    switch (kind) {
    case 1: hipLaunchKernelGGL((itw::decode_kernel<1>), grid, blk, 0, st, d_in, bx, (int32_t)n, d_out, d_stride, d_modes, width, height); break;
    case 3: hipLaunchKernelGGL((itw::decode_kernel<3>), grid, blk, 0, st, d_in, bx, (int32_t)n, d_out, d_stride, d_modes, width, height); break;
    case 7: hipLaunchKernelGGL((itw::decode_kernel<7>), grid, blk, 0, st, d_in, bx, (int32_t)n, d_out, d_stride, d_modes, width, height); break;
    case 4: hipLaunchKernelGGL((itw::decode_kernel<4>), grid, blk, 0, st, d_in, bx, (int32_t)n, d_out, d_stride, d_modes, width, height); break;
    case 5: hipLaunchKernelGGL((itw::decode_kernel<5>), grid, blk, 0, st, d_in, bx, (int32_t)n, d_out, d_stride, d_modes, width, height); break;
    case 14: hipLaunchKernelGGL((itw::decode_kernel<14>), grid, blk, 0, st, d_in, bx, (int32_t)n, d_out, d_stride, d_modes, width, height); break;
    case 15: hipLaunchKernelGGL((itw::decode_kernel<15>), grid, blk, 0, st, d_in, bx, (int32_t)n, d_out, d_stride, d_modes, width, height); break;
    default: hipLaunchKernelGGL((itw::decode_kernel<6>), grid, blk, 0, st, d_in, bx, (int32_t)n, d_out, d_stride, d_modes, width, height); break;
    }
    DEC_CHECK(hipGetLastError());
    if (!dout) DEC_CHECK(hipMemcpy2DAsync(out, (size_t)out_stride, d_out, row_bytes, row_bytes, (size_t)height, hipMemcpyDeviceToHost, st));
    if (modes && !dmodes) DEC_CHECK(hipMemcpyAsync(modes, d_modes, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (!din || !dout || !dmodes) {
        DEC_CHECK(hipStreamSynchronize(st));
        if (!din) (void)hipFree(d_in);
        if (!dout) (void)hipFree(d_out);
        if (modes && !dmodes) (void)hipFree(d_modes);
    }
    return 0;
}
