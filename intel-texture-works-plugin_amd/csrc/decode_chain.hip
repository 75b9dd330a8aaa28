// decode_chain.hip -- every image of a mip chain / cube map / array decoded in ONE launch (include/itw_decode.h: itwDecodeChain, itwDecodeImage):
// the mirror image of itwCompressImageChain.  itwDecodeBlocks, the older single-image entry, is a chain of one through the same kernel.
// The block decoder is decode_core.hpp's decode_block.  One block per lane: 8 / 16 B in, 64 B (RGBA8) or 128 B (RGBA16F) out, HBM bound
// by the output (4-8x the input).
//
// Lane = block of the chain's concatenated block list.  Its image is found by binary search over the first_block column of a small
// descriptor table, the search chain_gather_kernel (chain.hip) does; a wave may span several block rows and, in the tail of a chain, several
// whole images.  Stores are cropped to the image for every format: a block on the right / bottom edge writes min(4, w - 4x) x min(4, h - 4y)
// texels.  A row of a whole block goes out as one 16-B store (two for RGBA16F) at whatever dword address it has, the rows of a cropped block
// as dwords, so an output pointer or stride that is only 4-byte aligned works.  min_alpha[i] is the smallest alpha code among the texels stored for image i:
// a wave reduction per image the wave touches, then one atomicMin.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>
#include "../../include/itw_decode.h"
#include "../../include/itw_amd.h"
#include "decode_core.hpp"
#include "decode_chain_host.hpp"
#include "host_rt.hpp"

namespace itw {

// first on the stream, as measure_begin_kernel: every image's minimum starts at the largest word
__global__ void __launch_bounds__(256) decode_chain_begin_kernel(uint32_t* __restrict__ min_alpha, int32_t nimg)
{
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < nimg) min_alpha[i] = 0xFFFFFFFFu;
}

// Four dwords that go out as one 16-byte store.  Global memory takes a multi-dword store at any dword address, so a whole row of a block
// needs no more than the surface's own 4-byte alignment, and no test of it.
struct alignas(4) Dwords4 { uint32_t v[4]; };

// One block: decodes block j of the stream, stores the texels of it that lie inside `im`, returns the smallest alpha code among them
// (`want_min`: the caller asked for min_alpha; without it the decoded alphas are not looked at).
template <int FMT>
__device__ __forceinline__ uint32_t decode_chain_block(const uint8_t* __restrict__ blocks, const DecodeImage& im, int64_t j, int32_t* __restrict__ modes,
                                                       bool want_min)
{
    const int32_t b = (int32_t)(j - im.first_block);        // <= DECODE_IMAGE_MAX_BLOCKS
    const int32_t yy = b / im.blocks_x, xx = b - yy * im.blocks_x;
    const int ny = min(4, im.height - yy * 4), nx = min(4, im.width - xx * 4);
    const uint4 w = load_block<FMT>(blocks, j);
    int mode;
    const bool alpha = filled_alpha(FMT) < 0 && want_min;       // only the formats whose alpha is decoded, not filled, have a minimum to find
    uint32_t amin = filled_alpha(FMT) < 0 ? 0xFFFFFFFFu : (uint32_t)filled_alpha(FMT);
    uint8_t* o = im.ptr + (int64_t)yy * 4 * im.stride + (int64_t)xx * 4 * texel_bytes(FMT);
    const bool whole = nx == 4 && ny == 4;                      // an inner block: one branch for its four rows
    if constexpr (is_bc6h(FMT)) {
        uint32_t lo16[16], hi16[16];
        mode = decode_block<FMT>(w, lo16, hi16);
        if (whole) {
#pragma unroll
            for (int y = 0; y < 4; y++) {
                Dwords4* r4 = reinterpret_cast<Dwords4*>(o + y * im.stride);
                r4[0] = Dwords4{{lo16[y * 4], hi16[y * 4], lo16[y * 4 + 1], hi16[y * 4 + 1]}};
                r4[1] = Dwords4{{lo16[y * 4 + 2], hi16[y * 4 + 2], lo16[y * 4 + 3], hi16[y * 4 + 3]}};
            }
        } else
#pragma unroll
        for (int y = 0; y < 4; y++) {
            if (y >= ny) break;
            uint32_t* r1 = reinterpret_cast<uint32_t*>(o + y * im.stride);
#pragma unroll
            for (int x = 0; x < 4; x++) if (x < nx) { r1[2 * x] = lo16[y * 4 + x]; r1[2 * x + 1] = hi16[y * 4 + x]; }
        }
    } else {
        uint32_t px[16];
        mode = decode_block<FMT>(w, px);
        if (whole) {
#pragma unroll
            for (int y = 0; y < 4; y++) *reinterpret_cast<Dwords4*>(o + y * im.stride) = Dwords4{{px[y * 4], px[y * 4 + 1], px[y * 4 + 2], px[y * 4 + 3]}};
            if (alpha) {
#pragma unroll
                for (int k = 0; k < 16; k++) amin = min(amin, px[k] >> 24);
            }
        } else
#pragma unroll
        for (int y = 0; y < 4; y++) {
            if (y >= ny) break;
            uint32_t* r1 = reinterpret_cast<uint32_t*>(o + y * im.stride);
#pragma unroll
            for (int x = 0; x < 4; x++) if (x < nx) r1[x] = px[y * 4 + x];
            if (alpha) {
#pragma unroll
                for (int x = 0; x < 4; x++) if (x < nx) amin = min(amin, px[y * 4 + x] >> 24);
            }
        }
    }
    if (modes) modes[j] = mode;
    return amin;
}

// ONE: a chain of one image (itwDecodeImage, itwDecodeBlocks).  Its descriptor is the kernel argument `one` -- uniform, so the address arithmetic stays
// scalar -- and there is no table and no search.
template <int FMT, bool ONE>
__global__ void __launch_bounds__(256)
decode_chain_kernel(const uint8_t* __restrict__ blocks, const DecodeImage* __restrict__ images, const DecodeImage one, int32_t nimg, int64_t nblocks,
                    int32_t* __restrict__ modes, uint32_t* __restrict__ min_alpha)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = j < nblocks;                              // (no early return: the reduction below is wave-wide)
    int img = 0;
    uint32_t amin = 0xFFFFFFFFu;
    if (live) {
        if (ONE) {
            amin = decode_chain_block<FMT>(blocks, one, j, modes, min_alpha != nullptr);
        } else {
            int lo = 0, hi = nimg - 1;                          // the last image whose first block is <= j
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (images[mid].first_block <= j) lo = mid; else hi = mid - 1;
            }
            img = lo;
            const DecodeImage im = images[lo];
            amin = decode_chain_block<FMT>(blocks, im, j, modes, min_alpha != nullptr);
        }
    }
    if (!min_alpha) return;                                     // (a kernel argument: the whole wave leaves or stays)
    // per image the wave touches: the minimum over its lanes, then one atomic.  Images ascend with the lane, so each round retires the lowest
    const int lane = threadIdx.x & 63;
    bool pending = live;
    for (;;) {
        const unsigned long long todo = __ballot(pending);
        if (!todo) break;
        const int leader = __ffsll((long long)todo) - 1;
        const int cur = __shfl(img, leader);
        const bool mine = pending && img == cur;
        uint32_t v = mine ? amin : 0xFFFFFFFFu;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, off));
        if (lane == leader) atomicMin(&min_alpha[cur], v);
        if (mine) pending = false;
    }
}

} // namespace itw

namespace {

// everything that needs the device, for `who` (the entry point's name): the `count` images of `total` blocks that its checks have passed
void decode_chain(const char* who, int kind, const uint8_t* blocks, const rgba_surface* outs, int count, int64_t total, int32_t* modes,
                  uint32_t* min_alpha, bool douts)
{
    hipStream_t st = (hipStream_t)itwGetStream();
    const bool dblocks = itw::is_device_pointer(blocks), dmodes = !modes || itw::is_device_pointer(modes),
               dmin = !min_alpha || itw::is_device_pointer(min_alpha);
    if (dblocks && ((uintptr_t)blocks & 3)) itw::fail_msg("%s: device block stream at %p is not 4-byte aligned", who, (const void*)blocks);
    if ((dmodes && ((uintptr_t)modes & 3)) || (dmin && ((uintptr_t)min_alpha & 3))) itw::fail_msg("%s: misaligned modes / min_alpha", who);
    if ((total + 255) / 256 > (int64_t)0x7fffffff) itw::fail_msg("%s: %lld blocks are more than one launch covers", who, (long long)total);
    const size_t in_bytes = (size_t)total * (size_t)itw::block_bytes(kind);

    static thread_local std::vector<itw::DecodeImage> desc;     // grow-only, like the device buffer it is copied into
    desc.resize((size_t)count);
    itw::DecodeLayout L = itw::decode_chain_describe(kind, outs, count, total, nullptr, !dblocks, !douts, !dmodes, !dmin, desc.data());
    // a chain of one travels as a kernel argument: with everything on the device such a call touches no buffer of the thread at all
    const bool resident = dblocks && douts && dmodes && dmin, buffer = !(resident && count == 1);
    uint8_t* base = buffer ? static_cast<uint8_t*>(itw::decode_scratch(L.bytes, st)) : nullptr;
    if (!douts) L = itw::decode_chain_describe(kind, outs, count, total, base, !dblocks, true, !dmodes, !dmin, desc.data());

    // the table reaches the device the way compress_chain's does: one copy ahead of the launch, in stream order
    if (count > 1) ITW_CHECK(hipMemcpyAsync(base + L.desc, desc.data(), (size_t)count * sizeof(itw::DecodeImage), hipMemcpyHostToDevice, st));
    const uint8_t* d_blocks = blocks;
    if (!dblocks) { ITW_CHECK(hipMemcpyAsync(base + L.blocks, blocks, in_bytes, hipMemcpyHostToDevice, st)); d_blocks = base + L.blocks; }
    int32_t* d_modes = dmodes ? modes : reinterpret_cast<int32_t*>(base + L.modes);
    uint32_t* d_min = dmin ? min_alpha : reinterpret_cast<uint32_t*>(base + L.min_alpha);
    const itw::DecodeImage* d_desc = count > 1 ? reinterpret_cast<const itw::DecodeImage*>(base + L.desc) : nullptr;

    if (d_min) {
        hipLaunchKernelGGL(itw::decode_chain_begin_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, d_min, (int32_t)count);
        ITW_CHECK(hipGetLastError());
    }
    const dim3 grid((unsigned)((total + 255) / 256));
    itw::with_kind(kind, [&](auto K) {
        if (count == 1) hipLaunchKernelGGL((itw::decode_chain_kernel<K.value, true>), grid, dim3(256), 0, st, d_blocks, d_desc, desc[0], 1, total, d_modes, d_min);
        else hipLaunchKernelGGL((itw::decode_chain_kernel<K.value, false>), grid, dim3(256), 0, st, d_blocks, d_desc, desc[0], (int32_t)count, total, d_modes, d_min);
    });
    ITW_CHECK(hipGetLastError());
    if (resident) { if (buffer) itw::decode_scratch_done(st); return; }     // all on the device: asynchronous on the thread's stream

    if (!douts)
        for (int i = 0; i < count; i++) {                       // one strided download per image
            const size_t row_bytes = (size_t)outs[i].width * (size_t)itw::texel_bytes(kind);
            ITW_CHECK(hipMemcpy2DAsync(outs[i].ptr, (size_t)outs[i].stride, desc[(size_t)i].ptr, (size_t)desc[(size_t)i].stride, row_bytes,
                                       (size_t)outs[i].height, hipMemcpyDeviceToHost, st));
        }
    if (!dmodes) ITW_CHECK(hipMemcpyAsync(modes, d_modes, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    if (!dmin) ITW_CHECK(hipMemcpyAsync(min_alpha, d_min, (size_t)count * 4, hipMemcpyDeviceToHost, st));
    ITW_CHECK(hipStreamSynchronize(st));
    itw::decode_scratch_done(st);
}

} // namespace

extern "C" int itwDecodeChain(int dxgi_format, const uint8_t* blocks, const rgba_surface* outs, int count, int32_t* modes, uint32_t* min_alpha)
{
    dxgi_format = itw::stream_format(dxgi_format);                                // the BC1A codes: a BC1 stream
    const int kind = dxgi_format == 96 ? 0 : itw::decode_kind(dxgi_format);      // BC6H_SF16 stays refused: the signed reading goes by ITW_FORMAT_BC6H_SIGNED
    const int64_t total = itw::decode_chain_check(kind, blocks, outs, count);
    if (total <= 0) return total < 0 ? -1 : 0;
    const bool douts = itw::is_device_pointer(outs[0].ptr);
    for (int i = 1; i < count; i++)
        if (itw::is_device_pointer(outs[i].ptr) != douts) return -1;      // all host or all device, as the chain encoder asks
    const bool ok = itw::guarded([&] { decode_chain("itwDecodeChain", kind, blocks, outs, count, total, modes, min_alpha, douts); });
    return ok ? 0 : -1;
}

extern "C" int itwDecodeImage(int dxgi_format, const uint8_t* blocks, const rgba_surface* out, int32_t* modes, uint32_t* min_alpha)
{
    return itwDecodeChain(dxgi_format, blocks, out, 1, modes, min_alpha);
}

// The older single-image entry: its own argument rules (decode_blocks_check; 96 reads as unsigned), then a chain of one without min_alpha
extern "C" int itwDecodeBlocks(int dxgi_format, const uint8_t* blocks, int width, int height, uint8_t* out, int64_t out_stride, int32_t* modes)
{
    const int kind = itw::decode_kind(itw::stream_format(dxgi_format));
    const int64_t total = itw::decode_blocks_check(kind, width, height, out_stride);
    if (total < 0) return -1;
    const rgba_surface surface{out, width, height, (int32_t)out_stride};
    const bool ok = itw::guarded([&] {
        decode_chain("itwDecodeBlocks", kind, blocks, &surface, 1, total, modes, nullptr, itw::is_device_pointer(out));
    });
    return ok ? 0 : -1;
}
