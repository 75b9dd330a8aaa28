// refine.hip -- encode to an error budget (include/itw_dispatch.h: itwCompressImageRefined).  The whole surface is encoded with a cheap
// preset, every block is measured against its 16 source texels, and only the blocks whose error is above the caller's budget are encoded
// again with an expensive preset; a block takes the second encoding only where that is strictly better.  Blocks are independent, so every
// block written is the existing encoders' block -- the reference's -- under one of the two presets, and which of the two is an integer rule.
//
// On the stream, in order:
//   1. the first tier: the encoders' device-pointer path (abi.hip encode_resident), whole surface, into the (device copy of the) target;
//   2. refine_judge_kernel: one lane per block.  Decodes the block into registers (decode_core.hpp), loads its four source rows as vectors
//      (texel_rows.hpp), sums the squared differences of the channels in the mask -> error map, tier 0, and its workgroup's number of
//      listed blocks; sums and maxima by wave shuffles, LDS, one integer atomic per field per workgroup, as measure_kernel does;
//   3. refine_scan_kernel: one workgroup turns the per-workgroup counts into each workgroup's first list slot, and the total;
//      the host reads the total n through a pinned word -- the one synchronisation the call cannot do without;
//   4. refine_list_kernel: block b of workgroup g goes to slot first[g] + (listed blocks of g before b), by wave ballots.  The list is
//      therefore in ASCENDING block order whatever order the workgroups run in -- the gather reads the source front to back, and every
//      intermediate buffer of a call is the same bits on every run.  Counts plus a scan rather than a single pass with a look-back: no
//      workgroup ever waits for another one;
//   5. refine_gather_kernel: the listed blocks' texels into a packed surface of min(n, 256) blocks per row (the tail of the last row
//      repeats the last listed block: the encoder reads written texels only), one lane per texel row of a block as in chain.hip;
//   6. the refine tier over the packed surface, same path as 1., into scratch blocks;
//   7. refine_commit_kernel: one lane per listed block: decode, compare with the packed texels, apply the rule, store the winner;
//   8. refine_finish_kernel: one lane completes *stats.
// n == 0 skips 4. to 7.  Plain vector loads / stores and HIP atomics only.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/itw_dispatch.h"
#include "../../include/itw_decode.h"
#include "../../include/itw_amd.h"
#include "decode_core.hpp"
#include "texel_rows.hpp"
#include "host_rt.hpp"

static_assert(sizeof(itw_refine_stats) == 56, "itw_refine_stats layout");

namespace itw {

constexpr int REFINE_PACKED_BLOCKS = 256;                       // blocks per row of the packed surface

// what the kernels accumulate; refine_finish_kernel turns it into itw_refine_stats
struct RefineAcc {
    unsigned long long sse_first, worst_first;                  // judge: over every block
    unsigned long long worst_final;                             // judge: blocks off the list; commit: listed blocks, whichever encoding stays
    unsigned long long gained, replaced;                        // commit: sum of eA - eB over, and number of, the blocks that took B
    uint32_t listed, _pad;                                      // scan
};
static_assert(sizeof(RefineAcc) == 48, "refine_begin_kernel: one lane per dword");

// the error of the block `w` against the 4 x 4 texels at `p` (rows `stride` bytes apart): measure_kernel's per-block sum over the channels in `mask`
template <int FMT>
__device__ __forceinline__ unsigned long long refine_block_error(const uint4 w, const uint8_t* p, int64_t stride, uint32_t mask)
{
    if constexpr (FMT == BCN_BC6H) {
        uint32_t lo[16], hi[16];
        (void)decode_block<FMT>(w, lo, hi);
        unsigned long long e = 0ull;
#pragma unroll
        for (int y = 0; y < 4; y++) {
            uint32_t s[8];
            measure_load_row<8>(p + y * stride, 4, s);
#pragma unroll
            for (int x = 0; x < 4; x++) {
                const uint32_t d[2] = {lo[y * 4 + x], hi[y * 4 + x]};
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const int a = (int)((s[2 * x + (c >> 1)] >> (16 * (c & 1))) & 0xffffu), v = (int)((d[c >> 1] >> (16 * (c & 1))) & 0xffffu);
                    const uint32_t df = (uint32_t)abs(a - v);
                    e += ((mask >> c) & 1u) ? (unsigned long long)df * df : 0ull;
                }
            }
        }
        return e;
    } else {
        uint32_t px[16];
        (void)decode_block<FMT>(w, px);
        uint32_t e = 0u;                                        // 64 * 255^2 < 2^32
#pragma unroll
        for (int y = 0; y < 4; y++) {
            uint32_t s[4];
            measure_load_row<4>(p + y * stride, 4, s);
#pragma unroll
            for (int x = 0; x < 4; x++) {
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const int a = (int)((s[x] >> (8 * c)) & 255u), v = (int)((px[y * 4 + x] >> (8 * c)) & 255u);
                    const uint32_t df = (uint32_t)abs(a - v);
                    e += ((mask >> c) & 1u) ? df * df : 0u;
                }
            }
        }
        return (unsigned long long)e;
    }
}

__global__ void refine_begin_kernel(RefineAcc* __restrict__ acc)
{
    if (blockIdx.x == 0 && threadIdx.x < sizeof(RefineAcc) / 4) reinterpret_cast<uint32_t*>(acc)[threadIdx.x] = 0u;
}

// FMT: BCN_BC7 or BCN_BC6H (bcn_format.hpp).  `blocks`: 16-B aligned.
template <int FMT>
__global__ void __launch_bounds__(256)
refine_judge_kernel(const uint8_t* __restrict__ blocks, int32_t blocks_x, int32_t nblocks, const uint8_t* __restrict__ src, int64_t stride,
                    uint32_t mask, unsigned long long budget, unsigned long long* __restrict__ emap, uint8_t* __restrict__ tmap,
                    uint32_t* __restrict__ group_count, RefineAcc* __restrict__ acc)
{
    constexpr int PX = texel_bytes(FMT);
    __shared__ unsigned long long s_sum[4], s_max[4], s_stay[4];
    __shared__ uint32_t s_cnt[4];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int32_t b = (int32_t)blockIdx.x * 256 + t;
    unsigned long long e = 0ull;
    bool listed = false;
    if (b < nblocks) {
        const int32_t yy = b / blocks_x, xx = b - yy * blocks_x;
        const uint4 w = *reinterpret_cast<const uint4*>(blocks + (int64_t)b * 16);
        e = refine_block_error<FMT>(w, src + (int64_t)yy * 4 * stride + (int64_t)xx * 4 * PX, stride, mask);
        emap[b] = e;
        tmap[b] = 0;
        listed = e > budget;
    }
    const uint32_t cnt = (uint32_t)__popcll(__ballot(listed));
    const unsigned long long sum = wave_sum(e), mx = wave_max(e), stay = wave_max(listed ? 0ull : e);
    if (lane == 0) { s_sum[wave] = sum; s_max[wave] = mx; s_stay[wave] = stay; s_cnt[wave] = cnt; }
    __syncthreads();
    if (t == 0) {
        group_count[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    } else if (t == 1) {
        const unsigned long long v = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        if (v) atomicAdd(&acc->sse_first, v);
    } else if (t == 2) {
        const unsigned long long a = s_max[0] > s_max[1] ? s_max[0] : s_max[1], c = s_max[2] > s_max[3] ? s_max[2] : s_max[3];
        if (a | c) atomicMax(&acc->worst_first, a > c ? a : c);
    } else if (t == 3) {
        const unsigned long long a = s_stay[0] > s_stay[1] ? s_stay[0] : s_stay[1], c = s_stay[2] > s_stay[3] ? s_stay[2] : s_stay[3];
        if (a | c) atomicMax(&acc->worst_final, a > c ? a : c);
    }
}

// ONE workgroup: group_first[g] = listed blocks of the workgroups before g; their total -> acc->listed
__global__ void __launch_bounds__(256)
refine_scan_kernel(const uint32_t* __restrict__ group_count, int32_t groups, uint32_t* __restrict__ group_first, RefineAcc* __restrict__ acc)
{
    __shared__ uint32_t s_wave[4];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    uint32_t running = 0u;
    for (int32_t base = 0; base < groups; base += 256) {
        const int32_t g = base + t;
        const uint32_t v = g < groups ? group_count[g] : 0u;
        uint32_t inc = v;                                       // inclusive scan over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o); if (lane >= o) inc += u; }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        uint32_t before = 0u, total = 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) { const uint32_t wv = s_wave[k]; before += k < wave ? wv : 0u; total += wv; }
        if (g < groups) group_first[g] = running + before + inc - v;
        running += total;
        __syncthreads();
    }
    if (t == 0) acc->listed = running;
}

// the same 256 blocks per workgroup as the judge: list[group_first[g] + listed blocks of g before b] = b
__global__ void __launch_bounds__(256)
refine_list_kernel(const unsigned long long* __restrict__ emap, int32_t nblocks, unsigned long long budget, const uint32_t* __restrict__ group_first,
                   uint32_t* __restrict__ list)
{
    __shared__ uint32_t s_cnt[4];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int32_t b = (int32_t)blockIdx.x * 256 + t;
    const bool listed = b < nblocks && emap[b] > budget;
    const unsigned long long ballot = __ballot(listed);
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t before = 0u;
#pragma unroll
    for (int k = 0; k < 3; k++) before += k < wave ? s_cnt[k] : 0u;
    if (listed) list[group_first[blockIdx.x] + before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull))] = (uint32_t)b;
}

// PX: bytes per texel.  Slot j of the packed surface (`total` = packed_bx * block rows slots) = listed block min(j, n - 1).  64 slots per
// workgroup, wave r carrying texel row r: consecutive lanes write consecutive 4-texel pieces of one packed row.
template <int PX>
__global__ void __launch_bounds__(256)
refine_gather_kernel(const uint32_t* __restrict__ list, int32_t n, int32_t total, int32_t packed_bx, const uint8_t* __restrict__ src, int64_t stride,
                     int32_t blocks_x, uint8_t* __restrict__ dst, int64_t dst_pitch)
{
    const int r = threadIdx.x >> 6;
    const int32_t j = (int32_t)blockIdx.x * 64 + (threadIdx.x & 63);
    if (j >= total) return;
    const int32_t b = (int32_t)list[min(j, n - 1)];
    const int32_t yy = b / blocks_x, xx = b - yy * blocks_x;
    uint32_t v[PX];
    measure_load_row<PX>(src + ((int64_t)yy * 4 + r) * stride + (int64_t)xx * 4 * PX, 4, v);
    const int32_t prow = j / packed_bx, pcol = j - prow * packed_bx;
    uint4* out = reinterpret_cast<uint4*>(dst + ((int64_t)prow * 4 + r) * dst_pitch + (int64_t)pcol * 4 * PX);
#pragma unroll
    for (int q = 0; q < PX / 4; q++) out[q] = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}

// one lane per listed block: B = refined[i] against slot i of the packed surface; the rule; the winner into blocks / emap / tmap
template <int FMT>
__global__ void __launch_bounds__(256)
refine_commit_kernel(const uint32_t* __restrict__ list, int32_t n, int32_t packed_bx, const uint8_t* __restrict__ packed, int64_t pitch,
                     const uint8_t* __restrict__ refined, uint32_t mask, uint8_t* __restrict__ blocks, unsigned long long* __restrict__ emap,
                     uint8_t* __restrict__ tmap, RefineAcc* __restrict__ acc)
{
    constexpr int PX = texel_bytes(FMT);
    __shared__ unsigned long long s_gain[4], s_max[4];
    __shared__ uint32_t s_won[4];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int32_t i = (int32_t)blockIdx.x * 256 + t;
    unsigned long long gain = 0ull, fin = 0ull;
    uint32_t won = 0u;
    if (i < n) {
        const uint32_t b = list[i];
        const uint4 w = *reinterpret_cast<const uint4*>(refined + (int64_t)i * 16);
        const int32_t prow = i / packed_bx, pcol = i - prow * packed_bx;
        const unsigned long long eb = refine_block_error<FMT>(w, packed + (int64_t)prow * 4 * pitch + (int64_t)pcol * 4 * PX, pitch, mask);
        const unsigned long long ea = emap[b];
        if (eb < ea) {
            *reinterpret_cast<uint4*>(blocks + (int64_t)b * 16) = w;
            emap[b] = eb;
            tmap[b] = 2;
            gain = ea - eb; won = 1u; fin = eb;
        } else {
            tmap[b] = 1;
            fin = ea;
        }
    }
    gain = wave_sum(gain); won = wave_sum(won); fin = wave_max(fin);
    if (lane == 0) { s_gain[wave] = gain; s_won[wave] = won; s_max[wave] = fin; }
    __syncthreads();
    if (t == 0) {
        const unsigned long long v = s_gain[0] + s_gain[1] + s_gain[2] + s_gain[3];
        if (v) atomicAdd(&acc->gained, v);
    } else if (t == 1) {
        const unsigned long long v = (unsigned long long)s_won[0] + s_won[1] + s_won[2] + s_won[3];
        if (v) atomicAdd(&acc->replaced, v);
    } else if (t == 2) {
        const unsigned long long a = s_max[0] > s_max[1] ? s_max[0] : s_max[1], c = s_max[2] > s_max[3] ? s_max[2] : s_max[3];
        if (a | c) atomicMax(&acc->worst_final, a > c ? a : c);
    }
}

__global__ void refine_finish_kernel(const RefineAcc* __restrict__ acc, unsigned long long nblocks, itw_refine_stats* __restrict__ stats)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    stats->blocks = nblocks;
    stats->listed = acc->listed;
    stats->replaced = acc->replaced;
    stats->sse_first = acc->sse_first;
    stats->sse_final = acc->sse_first - acc->gained;
    stats->worst_first = acc->worst_first;
    stats->worst_final = acc->worst_final;
}

} // namespace itw

namespace {

// offsets into a scratch buffer, each a multiple of 256
struct Carve {
    size_t used = 0;
    size_t take(size_t bytes) { const size_t at = used; used += (bytes + 255) & ~(size_t)255; return at; }
};

// everything that needs the device
void refine(int kind, const rgba_surface& s, uint8_t* target, int dxgi_format, const void* first, const void* second, uint32_t mask,
            uint64_t budget, itw_refine_stats* stats, uint64_t* block_sse, uint8_t* tier_map)
{
    using namespace itw;
    hipStream_t st = (hipStream_t)itwGetStream();
    const int px = texel_bytes(kind);
    const int bx = s.width / 4, by = s.height / 4;
    const int64_t nb = (int64_t)bx * by;
    const int32_t groups = (int32_t)((nb + 255) / 256);
    const size_t row_bytes = (size_t)s.width * px, src_pitch = (row_bytes + 15) & ~(size_t)15;
    // the kernels take device memory; the judge and the commit load and store whole blocks as 16-B vectors
    const bool dsrc = is_device_pointer(s.ptr), dtgt = is_device_pointer(target) && ((uintptr_t)target & 15) == 0,
               dstats = is_device_pointer(stats), dmap = block_sse && is_device_pointer(block_sse), dtier = tier_map && is_device_pointer(tier_map);

    Carve c0;
    const size_t o_acc = c0.take(sizeof(RefineAcc)), o_stats = c0.take(sizeof(itw_refine_stats)), o_count = c0.take((size_t)groups * 4),
                 o_first = c0.take((size_t)groups * 4), o_list = c0.take((size_t)nb * 4), o_src = c0.take(dsrc ? 0 : src_pitch * (size_t)s.height),
                 o_tgt = c0.take(dtgt ? 0 : (size_t)nb * 16), o_map = c0.take(dmap ? 0 : (size_t)nb * 8), o_tier = c0.take(dtier ? 0 : (size_t)nb);
    uint8_t* base = static_cast<uint8_t*>(refine_scratch(0, c0.used));
    RefineAcc* acc = reinterpret_cast<RefineAcc*>(base + o_acc);
    itw_refine_stats* d_stats = dstats ? stats : reinterpret_cast<itw_refine_stats*>(base + o_stats);
    uint32_t* group_count = reinterpret_cast<uint32_t*>(base + o_count);
    uint32_t* group_first = reinterpret_cast<uint32_t*>(base + o_first);
    uint32_t* list = reinterpret_cast<uint32_t*>(base + o_list);
    uint8_t* d_tgt = dtgt ? target : base + o_tgt;
    unsigned long long* d_map = reinterpret_cast<unsigned long long*>(dmap ? reinterpret_cast<uint8_t*>(block_sse) : base + o_map);
    uint8_t* d_tier = dtier ? tier_map : base + o_tier;
    uint32_t* host_n = refine_count_word();

    // a failure below is a C++ exception: what the call has queued by then is drained, so that the next call finds the scratch idle
    struct Unwind { bool done; hipStream_t st; ~Unwind() { if (!done) { (void)hipStreamSynchronize(st); (void)hipGetLastError(); } } } unwind{false, st};

    const uint8_t* d_src = s.ptr;
    int64_t stride = s.stride;
    if (!dsrc) {
        ITW_CHECK(hipMemcpy2DAsync(base + o_src, src_pitch, s.ptr, (size_t)s.stride, row_bytes, (size_t)s.height, hipMemcpyHostToDevice, st));
        d_src = base + o_src; stride = (int64_t)src_pitch;
    }
    encode_resident(dxgi_format, first, d_src, stride, s.width, s.height, d_tgt);

    const dim3 blk(256);
    hipLaunchKernelGGL(refine_begin_kernel, dim3(1), dim3(64), 0, st, acc);
    ITW_CHECK(hipGetLastError());
    if (kind == BCN_BC7) hipLaunchKernelGGL((refine_judge_kernel<BCN_BC7>), dim3((unsigned)groups), blk, 0, st, d_tgt, bx, (int32_t)nb, d_src, stride, mask,
                                      (unsigned long long)budget, d_map, d_tier, group_count, acc);
    else           hipLaunchKernelGGL((refine_judge_kernel<BCN_BC6H>), dim3((unsigned)groups), blk, 0, st, d_tgt, bx, (int32_t)nb, d_src, stride, mask,
                                      (unsigned long long)budget, d_map, d_tier, group_count, acc);
    ITW_CHECK(hipGetLastError());
    hipLaunchKernelGGL(refine_scan_kernel, dim3(1), blk, 0, st, group_count, groups, group_first, acc);
    ITW_CHECK(hipGetLastError());
    ITW_CHECK(hipMemcpyAsync(host_n, &acc->listed, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    ITW_CHECK(hipStreamSynchronize(st));
    const int64_t n = (int64_t)*host_n;
    if (n < 0 || n > nb) fail_msg("itwCompressImageRefined: %lld blocks listed of %lld", (long long)n, (long long)nb);

    if (n > 0) {
        const int32_t pbx = (int32_t)(n < REFINE_PACKED_BLOCKS ? n : REFINE_PACKED_BLOCKS), pby = (int32_t)((n + pbx - 1) / pbx);
        const int32_t total = pbx * pby;
        const int64_t pitch = (int64_t)pbx * 4 * px;
        Carve c1;
        const size_t o_packed = c1.take((size_t)pitch * 4 * pby), o_refined = c1.take((size_t)total * 16);
        uint8_t* lbase = static_cast<uint8_t*>(refine_scratch(1, c1.used));
        uint8_t* packed = lbase + o_packed;
        uint8_t* refined = lbase + o_refined;
        hipLaunchKernelGGL(refine_list_kernel, dim3((unsigned)groups), blk, 0, st, d_map, (int32_t)nb, (unsigned long long)budget, group_first, list);
        ITW_CHECK(hipGetLastError());
        const dim3 ggrid((unsigned)((total + 63) / 64));
        if (kind == BCN_BC7) hipLaunchKernelGGL((refine_gather_kernel<4>), ggrid, blk, 0, st, list, (int32_t)n, total, pbx, d_src, stride, bx, packed, pitch);
        else           hipLaunchKernelGGL((refine_gather_kernel<8>), ggrid, blk, 0, st, list, (int32_t)n, total, pbx, d_src, stride, bx, packed, pitch);
        ITW_CHECK(hipGetLastError());
        encode_resident(dxgi_format, second, packed, pitch, pbx * 4, pby * 4, refined);
        const dim3 cgrid((unsigned)((n + 255) / 256));
        if (kind == BCN_BC7) hipLaunchKernelGGL((refine_commit_kernel<BCN_BC7>), cgrid, blk, 0, st, list, (int32_t)n, pbx, packed, pitch, refined, mask, d_tgt, d_map, d_tier, acc);
        else           hipLaunchKernelGGL((refine_commit_kernel<BCN_BC6H>), cgrid, blk, 0, st, list, (int32_t)n, pbx, packed, pitch, refined, mask, d_tgt, d_map, d_tier, acc);
        ITW_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(refine_finish_kernel, dim3(1), dim3(64), 0, st, acc, (unsigned long long)nb, d_stats);
    ITW_CHECK(hipGetLastError());

    if (!dtgt) ITW_CHECK(hipMemcpyAsync(target, d_tgt, (size_t)nb * 16, hipMemcpyDefault, st));
    if (!dstats) ITW_CHECK(hipMemcpyAsync(stats, d_stats, sizeof(itw_refine_stats), hipMemcpyDeviceToHost, st));
    if (block_sse && !dmap) ITW_CHECK(hipMemcpyAsync(block_sse, d_map, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
    if (tier_map && !dtier) ITW_CHECK(hipMemcpyAsync(tier_map, d_tier, (size_t)nb, hipMemcpyDeviceToHost, st));
    ITW_CHECK(hipStreamSynchronize(st));
    unwind.done = true;
}

} // namespace

extern "C" bool itwCompressImageRefined(const rgba_surface* source, uint8_t* target, int dxgi_format, const void* first_settings,
                                        const void* refine_settings, uint32_t channel_mask, uint64_t max_block_sse, itw_refine_stats* stats,
                                        size_t stats_bytes, uint64_t* block_sse, uint8_t* tier_map)
{
    itw::clear_failure();
    return itw::guarded([&] {
        // the checks that need no device
        const int kind = itw::decode_kind(dxgi_format);
        if (kind != itw::BCN_BC7 && kind != itw::BCN_BC6H) itw::fail_msg("itwCompressImageRefined: DXGI format %d has one encoder only (BC7 and BC6H have presets to refine with)", dxgi_format);
        if (!source || !source->ptr || !target) itw::fail_msg("itwCompressImageRefined: null surface, texel or target pointer");
        if (!first_settings || !refine_settings) itw::fail_msg("itwCompressImageRefined: null settings for the %s tier", first_settings ? "refine" : "first");
        if (!stats) itw::fail_msg("itwCompressImageRefined: null stats");
        if (stats_bytes != sizeof(itw_refine_stats))
            itw::fail_msg("itwCompressImageRefined: stats_bytes %zu != sizeof(itw_refine_stats) = %zu", stats_bytes, sizeof(itw_refine_stats));
        if (((uintptr_t)stats & 7) || ((uintptr_t)block_sse & 7)) itw::fail_msg("itwCompressImageRefined: stats and block_sse must be 8-byte aligned");
        if (channel_mask == 0 || channel_mask > 15) itw::fail_msg("itwCompressImageRefined: channel mask %u (1..15: bit 0 = R .. bit 3 = A)", channel_mask);
        if (source->width < 4 || source->height < 4 || (source->width & 3) || (source->height & 3))
            itw::fail_msg("itwCompressImageRefined: %d x %d: width and height must be multiples of 4 (itwPadToMultipleOf4)", source->width, source->height);
        const int64_t row = (int64_t)source->width * itw::texel_bytes(kind);
        if ((int64_t)source->stride < row) itw::fail_msg("itwCompressImageRefined: stride %d < %lld bytes per row", source->stride, (long long)row);
        if ((int64_t)(source->width / 4) * (source->height / 4) > (int64_t)ITW_MEASURE_MAX_BLOCKS)
            itw::fail_msg("itwCompressImageRefined: %d x %d is more than %lld blocks", source->width, source->height, (long long)ITW_MEASURE_MAX_BLOCKS);
        refine(kind, *source, target, dxgi_format, first_settings, refine_settings, channel_mask, max_block_sse, stats, block_sse, tier_map);
    });
}
