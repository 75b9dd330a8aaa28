// measure.hip -- how far an encoded stream is from its source, on the device (include/itw_decode.h: itwMeasureBlocks, itwMeasureChain,
// itwStatsPsnr).  Decode, compare and reduce in ONE kernel: the decoded surface never exists in memory.  One lane per block, as in
// decode_chain_kernel: 8 / 16 B of block in, its up-to-4x4 source texels in as row-wide vector loads (16 B per RGBA8 row, 2 x 16 B per RGBA16F
// row; rows and columns of partial edge blocks guarded), decoded into registers by decode_core.hpp's decode_block, and compared code by
// code.  Every quantity is an integer, so the result is the same bits on every run.
//
// Reduction.  A workgroup walks the block list with a grid stride (at most MEASURE_MAX_GROUPS workgroups, so that the handful of atomics
// a workgroup ends in stay few however large the surface), each lane keeping four sums and four maxima in registers; then wave64
// shuffles, the workgroup's four waves through LDS, and the first lanes of wave 0 issue the 64-bit integer atomicAdd / atomicMax into
// *stats (zeroed by measure_begin_kernel, first on the stream), one field per lane.  Integer atomics commute.  The worst block is an ordered arg-max: (block sse << 25 | inverted raster index)
// as one 64-bit atomicMax key kept in the worst_block_sse field, which measure_finish_kernel -- one lane, next on the stream -- splits
// into worst_block_sse / worst_block and completes with the header fields.  64 * 0xFFFF^2 < 2^39 (BC6H's largest block), which leaves 25
// index bits: ITW_MEASURE_MAX_BLOCKS.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <limits>
#include <type_traits>
#include <vector>
#include "../../include/itw_decode.h"
#include "../../include/itw_amd.h"
#include "decode_core.hpp"
#include "texel_rows.hpp"
#include "host_rt.hpp"

static_assert(sizeof(itw_error_stats) == 216, "itw_error_stats layout");

namespace itw {

constexpr int MEASURE_INDEX_BITS = 25;
constexpr uint32_t MEASURE_INDEX_MASK = (1u << MEASURE_INDEX_BITS) - 1u;
constexpr int MEASURE_MAX_GROUPS = 1024;      // 4 workgroups per CU; <= 2^25 / (1024 * 256) = 128 blocks per lane: 128 * 16 * 255^2 < 2^32
static_assert((uint64_t)ITW_MEASURE_MAX_BLOCKS == (1ull << MEASURE_INDEX_BITS), "the key's index field is what limits the block count");

// FMT: a BcnKind (bcn_format.hpp).  `blocks` is 16-byte aligned (8 for the 8-byte formats).  The SNORM pair compares int8 codes, a source
// code of -128 read as -127 (both are -1.0; the decoder never emits -128).  BCN_BC6HS compares sign-and-magnitude codes (itw_decode.h): a
// difference is at most 0xFFFE, so the block sums keep to the unsigned reading's bound
template <int FMT>
__global__ void __launch_bounds__(256)
measure_kernel(const uint8_t* __restrict__ blocks, int32_t blocks_x, int32_t nblocks, const uint8_t* __restrict__ src, int64_t stride,
               int32_t width, int32_t height, itw_error_stats* __restrict__ stats, unsigned long long* __restrict__ block_sse)
{
    using Acc = typename std::conditional<is_bc6h(FMT), unsigned long long, uint32_t>::type;   // a lane's per-channel sum: 16 * 0xFFFF^2 > 2^32 for BC6H
    __shared__ unsigned long long s_sum[4][4], s_key[4];
    __shared__ uint32_t s_max[4][4], s_hist[17];               // [16]: reserved-prefix blocks
    const int t = threadIdx.x;
    if (t < 17) s_hist[t] = 0u;
    __syncthreads();

    Acc sum[4] = {0, 0, 0, 0};
    uint32_t mx[4] = {0u, 0u, 0u, 0u};
    unsigned long long key = 0ull;
    uint32_t mine = 0u;                                         // blocks this lane measured (formats without modes)
    for (int32_t b = blockIdx.x * 256 + t; b < nblocks; b += gridDim.x * 256) {
        const int32_t yy = b / blocks_x, xx = b - yy * blocks_x;
        const int ny = min(4, height - yy * 4), nx = min(4, width - xx * 4);
        Acc bs[4] = {0, 0, 0, 0};
        uint4 w;
        if constexpr (block_bytes(FMT) == 8) { const uint2 v = *reinterpret_cast<const uint2*>(blocks + (int64_t)b * 8); w = make_uint4(v.x, v.y, 0u, 0u); }
        else w = *reinterpret_cast<const uint4*>(blocks + (int64_t)b * 16);
        int mode;
        if constexpr (is_bc6h(FMT)) {
            uint32_t lo[16], hi[16];
            mode = decode_block<FMT>(w, lo, hi);
            const uint8_t* p = src + (int64_t)yy * 4 * stride + (int64_t)xx * 32;
#pragma unroll
            for (int y = 0; y < 4; y++) {
                if (y >= ny) break;
                uint32_t s[8];
                measure_load_row<8>(p + y * stride, nx, s);
#pragma unroll
                for (int x = 0; x < 4; x++) {
                    if (x >= nx) continue;
                    const uint32_t d[2] = {lo[y * 4 + x], hi[y * 4 + x]};
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        int a = (int)((s[2 * x + (c >> 1)] >> (16 * (c & 1))) & 0xffffu), e = (int)((d[c >> 1] >> (16 * (c & 1))) & 0xffffu);
                        if constexpr (FMT == BCN_BC6HS) {       // the integer the signed reading interpolates in: sign bit and magnitude, both zeros 0
                            a = (a & 0x8000) ? -(a & 0x7FFF) : a;
                            e = (e & 0x8000) ? -(e & 0x7FFF) : e;
                        }
                        const uint32_t df = (uint32_t)abs(a - e);
                        bs[c] += (unsigned long long)df * df;
                        mx[c] = max(mx[c], df);
                    }
                }
            }
        } else {
            uint32_t px[16];
            mode = decode_block<FMT>(w, px);
            const uint8_t* p = src + (int64_t)yy * 4 * stride + (int64_t)xx * 16;
#pragma unroll
            for (int y = 0; y < 4; y++) {
                if (y >= ny) break;
                uint32_t s[4];
                measure_load_row<4>(p + y * stride, nx, s);
#pragma unroll
                for (int x = 0; x < 4; x++) {
                    if (x >= nx) continue;
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        int a = (int)((s[x] >> (8 * c)) & 255u), e = (int)((px[y * 4 + x] >> (8 * c)) & 255u);
                        if (FMT == BCN_BC4S || FMT == BCN_BC5S) { a = max((int)(int8_t)a, -127); e = (int)(int8_t)e; }
                        const uint32_t df = (uint32_t)abs(a - e);
                        bs[c] += df * df;
                        mx[c] = max(mx[c], df);
                    }
                }
            }
        }
        const unsigned long long total = (unsigned long long)bs[0] + bs[1] + bs[2] + bs[3];
        if (block_sse) block_sse[b] = total;
        const unsigned long long k = (total << MEASURE_INDEX_BITS) | (unsigned long long)(MEASURE_INDEX_MASK - (uint32_t)b);
        key = k > key ? k : key;
#pragma unroll
        for (int c = 0; c < 4; c++) sum[c] += bs[c];
        if (has_modes(FMT)) atomicAdd(&s_hist[mode < 0 ? 16 : mode], 1u);
        else mine++;
    }

    // wave64 -> the workgroup's waves through LDS -> one atomic per field
    const int wave = t >> 6, lane = t & 63;
    unsigned long long ws[4];
    uint32_t wm[4];
#pragma unroll
    for (int c = 0; c < 4; c++) { ws[c] = wave_sum((unsigned long long)sum[c]); wm[c] = wave_max(mx[c]); }
    key = wave_max(key);
    if (!has_modes(FMT)) mine = wave_sum(mine);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 4; c++) { s_sum[wave][c] = ws[c]; s_max[wave][c] = wm[c]; }
        s_key[wave] = key;
        if (!has_modes(FMT)) atomicAdd(&s_hist[0], mine);
    }
    __syncthreads();
    if (t < 20) {                                               // lanes 0-3: sse[], 4-19: mode_hist[]
        const unsigned long long v = t < 4 ? s_sum[0][t] + s_sum[1][t] + s_sum[2][t] + s_sum[3][t] : (unsigned long long)s_hist[t - 4];
        unsigned long long* dst = t < 4 ? reinterpret_cast<unsigned long long*>(&stats->sse[t]) : reinterpret_cast<unsigned long long*>(&stats->mode_hist[t - 4]);
        if (v) atomicAdd(dst, v);
    } else if (t < 24) {
        const int c = t - 20;
        const uint32_t v = max(max(s_max[0][c], s_max[1][c]), max(s_max[2][c], s_max[3][c]));
        if (v) atomicMax(&stats->max_abs[c], v);
    } else if (t == 24) {
        const unsigned long long a = s_key[0] > s_key[1] ? s_key[0] : s_key[1], c = s_key[2] > s_key[3] ? s_key[2] : s_key[3];
        atomicMax(reinterpret_cast<unsigned long long*>(&stats->worst_block_sse), a > c ? a : c);
    } else if (t == 25) {
        if (s_hist[16]) atomicAdd(&stats->reserved_blocks, s_hist[16]);
    }
}

// first on the stream: every accumulator of *stats starts at zero.  A kernel and not hipMemsetAsync, so that a captured call is three kernel
// nodes and nothing whose replay depends on how the runtime builds a memset node.
__global__ void measure_begin_kernel(itw_error_stats* __restrict__ stats)
{
    constexpr int DWORDS = (int)(sizeof(itw_error_stats) / 4);
    if (blockIdx.x == 0 && threadIdx.x < DWORDS) reinterpret_cast<uint32_t*>(stats)[threadIdx.x] = 0u;
}

// last on the stream: the arg-max key becomes the two worst-block fields, and the header fields are filled in
__global__ void measure_finish_kernel(itw_error_stats* __restrict__ stats, int32_t dxgi_format, int32_t width, int32_t height, unsigned long long nblocks)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long key = stats->worst_block_sse;
    stats->worst_block_sse = key >> MEASURE_INDEX_BITS;
    stats->worst_block = MEASURE_INDEX_MASK - (uint32_t)(key & MEASURE_INDEX_MASK);
    stats->_pad = 0u;
    stats->dxgi_format = dxgi_format; stats->width = width; stats->height = height;
    stats->blocks = nblocks;
}

} // namespace itw

namespace {

// the checks that need no device
bool surface_ok(int kind, const rgba_surface* s)
{
    if (!s || !s->ptr || s->width < 1 || s->height < 1) return false;
    if ((int64_t)s->stride < (int64_t)s->width * itw::texel_bytes(kind)) return false;
    return itw::image_blocks(*s) <= (int64_t)ITW_MEASURE_MAX_BLOCKS;
}

// everything on the device: three kernels -- zero, measure, finish -- in stream order; allocates nothing
void enqueue(int kind, int dxgi_format, const uint8_t* d_blocks, const uint8_t* d_src, int64_t stride, int width, int height,
             itw_error_stats* d_stats, uint64_t* d_map, hipStream_t st)
{
    const int bx = (width + 3) / 4;
    const int64_t n = (int64_t)bx * ((height + 3) / 4);               // <= ITW_MEASURE_MAX_BLOCKS (surface_ok)
    const int64_t groups = (n + 255) / 256;
    const dim3 grid((unsigned)(groups < itw::MEASURE_MAX_GROUPS ? groups : itw::MEASURE_MAX_GROUPS)), blk(256);
    unsigned long long* map = reinterpret_cast<unsigned long long*>(d_map);
    static_assert(sizeof(itw_error_stats) / 4 <= 64, "measure_begin_kernel: one lane per dword");
    hipLaunchKernelGGL(itw::measure_begin_kernel, dim3(1), dim3(64), 0, st, d_stats);
    ITW_CHECK(hipGetLastError());
    itw::with_kind(kind, [&](auto K) {
        hipLaunchKernelGGL((itw::measure_kernel<K.value>), grid, blk, 0, st, d_blocks, bx, (int32_t)n, d_src, stride, width, height, d_stats, map);
    });
    ITW_CHECK(hipGetLastError());
    hipLaunchKernelGGL(itw::measure_finish_kernel, dim3(1), dim3(64), 0, st, d_stats, (int32_t)dxgi_format, (int32_t)width, (int32_t)height, (unsigned long long)n);
    ITW_CHECK(hipGetLastError());
}

// device copies of a call's host-pointer arguments; freed when the call ends (after its synchronise)
struct Staging {
    std::vector<void*> bufs;
    ~Staging() { for (void* p : bufs) (void)hipFree(p); }
    void* alloc(size_t bytes)
    {
        void* p = nullptr;
        ITW_CHECK(hipMalloc(&p, bytes ? bytes : 1));
        bufs.push_back(p);
        return p;
    }
    const uint8_t* upload(const uint8_t* host, size_t bytes, hipStream_t st)
    {
        void* d = alloc(bytes);
        ITW_CHECK(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, st));
        return static_cast<const uint8_t*>(d);
    }
    const uint8_t* upload_rows(const rgba_surface& s, size_t row_bytes, hipStream_t st)
    {
        void* d = alloc(row_bytes * (size_t)s.height);
        ITW_CHECK(hipMemcpy2DAsync(d, row_bytes, s.ptr, (size_t)s.stride, row_bytes, (size_t)s.height, hipMemcpyHostToDevice, st));
        return static_cast<const uint8_t*>(d);
    }
};

} // namespace

extern "C" int itwMeasureBlocks(int dxgi_format, const uint8_t* blocks, const rgba_surface* source, itw_error_stats* stats, size_t stats_bytes,
                                uint64_t* block_sse)
{
    dxgi_format = itw::stream_format(dxgi_format);            // the BC1A codes: a BC1 stream, measured (and reported in `stats`) as 71 / 72
    const int kind = itw::decode_kind(dxgi_format);
    if (!kind || !blocks || !stats || stats_bytes != sizeof(itw_error_stats) || !surface_ok(kind, source)) return -1;
    if (((uintptr_t)stats & 7) || ((uintptr_t)block_sse & 7)) return -1;
    const bool ok = itw::guarded([&] {
        hipStream_t st = (hipStream_t)itwGetStream();
        const bool dblocks = itw::is_device_pointer(blocks), dsrc = itw::is_device_pointer(source->ptr), dstats = itw::is_device_pointer(stats),
                   dmap = !block_sse || itw::is_device_pointer(block_sse);
        const int64_t n = itw::image_blocks(*source);
        const size_t row_bytes = (size_t)source->width * itw::texel_bytes(kind);
        Staging tmp;
        const uint8_t* d_blocks = dblocks ? blocks : tmp.upload(blocks, (size_t)n * itw::block_bytes(kind), st);
        const uint8_t* d_src = dsrc ? source->ptr : tmp.upload_rows(*source, row_bytes, st);
        itw_error_stats* d_stats = dstats ? stats : static_cast<itw_error_stats*>(tmp.alloc(sizeof(itw_error_stats)));
        uint64_t* d_map = dmap ? block_sse : static_cast<uint64_t*>(tmp.alloc((size_t)n * 8));
        enqueue(kind, dxgi_format, d_blocks, d_src, dsrc ? (int64_t)source->stride : (int64_t)row_bytes, source->width, source->height, d_stats, d_map, st);
        if (dblocks && dsrc && dstats && dmap) return;          // all on the device: asynchronous on the thread's stream
        if (!dstats) ITW_CHECK(hipMemcpyAsync(stats, d_stats, sizeof(itw_error_stats), hipMemcpyDeviceToHost, st));
        if (!dmap) ITW_CHECK(hipMemcpyAsync(block_sse, d_map, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        ITW_CHECK(hipStreamSynchronize(st));
    });
    return ok ? 0 : -1;
}

extern "C" int itwMeasureChain(const rgba_surface* images, int count, const uint8_t* blocks, int dxgi_format, itw_error_stats* stats, size_t stats_bytes)
{
    dxgi_format = itw::stream_format(dxgi_format);
    const int kind = itw::decode_kind(dxgi_format);
    if (!kind || !images || count < 1 || !blocks || !stats || stats_bytes != sizeof(itw_error_stats) || ((uintptr_t)stats & 7)) return -1;
    int64_t total = 0;
    for (int i = 0; i < count; i++) {
        if (!surface_ok(kind, &images[i])) return -1;
        total += itw::image_blocks(images[i]);
    }
    const bool ok = itw::guarded([&] {
        hipStream_t st = (hipStream_t)itwGetStream();
        const bool dblocks = itw::is_device_pointer(blocks), dsrc = itw::all_one_pointer_kind("itwMeasureChain", "image", images, count),
                   dstats = itw::is_device_pointer(stats);
        Staging tmp;
        const uint8_t* d_blocks = dblocks ? blocks : tmp.upload(blocks, (size_t)total * itw::block_bytes(kind), st);
        itw_error_stats* d_stats = dstats ? stats : static_cast<itw_error_stats*>(tmp.alloc(sizeof(itw_error_stats) * (size_t)count));
        int64_t first = 0;                                      // image i's blocks start where the images before it end (itwChainBytes)
        for (int i = 0; i < count; i++) {
            const rgba_surface& im = images[i];
            const size_t row_bytes = (size_t)im.width * itw::texel_bytes(kind);
            const uint8_t* d_src = dsrc ? im.ptr : tmp.upload_rows(im, row_bytes, st);
            enqueue(kind, dxgi_format, d_blocks + first * itw::block_bytes(kind), d_src, dsrc ? (int64_t)im.stride : (int64_t)row_bytes, im.width, im.height,
                    d_stats + i, nullptr, st);
            first += itw::image_blocks(im);
        }
        if (dblocks && dsrc && dstats) return;
        if (!dstats) ITW_CHECK(hipMemcpyAsync(stats, d_stats, sizeof(itw_error_stats) * (size_t)count, hipMemcpyDeviceToHost, st));
        ITW_CHECK(hipStreamSynchronize(st));
    });
    return ok ? 0 : -1;
}

extern "C" double itwStatsPsnr(const itw_error_stats* stats, uint32_t channel_mask)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int kind = stats ? itw::decode_kind(itw::stream_format(stats->dxgi_format)) : 0;
    if (!stats || !(channel_mask & 15u) || itw::is_bc6h(kind)) return nan;
    double sum = 0.0;
    int channels = 0;
    for (int c = 0; c < 4; c++)
        if (channel_mask & (1u << c)) { sum += (double)stats->sse[c]; channels++; }
    if (sum == 0.0) return std::numeric_limits<double>::infinity();
    const double n = (double)stats->width * (double)stats->height * (double)channels;
    const double peak = (kind == itw::BCN_BC4S || kind == itw::BCN_BC5S) ? 254.0 : 255.0;      // int8 codes -127..127
    return 10.0 * std::log10(peak * peak * n / sum);
}
