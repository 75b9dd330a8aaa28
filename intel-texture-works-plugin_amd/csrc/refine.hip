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
//
// itwCompressImageRefinedTo: the caller gives a number of blocks or a summed error to reach, and the budget is chosen on the device from
// the error map the judge left there.  The judge runs with budget UINT64_MAX (nothing listed); then, per round:
//   a. refine_round_begin_kernel: clears the select's histograms and state; for a target, sets acc->met once the stream's summed error
//      is at or below it -- every kernel of the round up to the scan then returns at once, and the host ends the call on that word;
//   b. the select: T = the (k+1)-th largest error among the blocks still at tier 0, 0 if there are at most k.  A radix select from the
//      top digit down, SELECT_BITS per pass: select_hist_kernel counts the digit of the candidates that share the digits chosen so far
//      (per-workgroup histogram in LDS, one atomic per wave where the wave's candidates agree, non-empty bins flushed with one global
//      atomic each), select_scan_kernel (ONE workgroup) walks the bins from the top, chooses the digit that holds the rank and leaves the
//      prefix and the rank inside that bin for the next pass.  Every pass is enqueued up front; a pass whose digit lies above
//      acc->worst_first returns at once (its digit is 0 for every block).  Counts are integers and T is a value: the order in which the
//      atomics land cannot change it;
//   c. refine_count_kernel: the judge's 256 blocks per workgroup; listed = tier 0 and error > T, T read from the device; group counts.
//      The largest error among the blocks that stay is T itself (refine_finish_to_kernel);
//   d. 3. to 7. as above, the list kernel taking T by pointer and the tier filter.  The host reads acc->met next to acc->listed.
//
// itwCompressImageChainRefined[To]: the same core behind a second front door.  The core reads a VIEW -- a device surface, its stride, its
// blocks per row, a block count and, optionally, one byte of extent per block -- and not an rgba_surface.  A single image is viewed in
// place, without a table: the path above, the non-CROP kernels.  A chain is gathered once, whole, with edge replication, into one packed
// surface of min(1024, n) blocks per row (chain.hip: the encoders then see what itwCompressImageChainEx shows them), the gather also
// writing each block's extent (pw - 1) | (ph - 1) << 2; the first tier encodes the packed surface into scratch (its last row may run
// past n) and the first n blocks are copied out at the end.  The judge and the commit take the CROP variant of the block error, which
// leaves the replicated padding out -- itwMeasureBlocks' block_sse of the image.  Everything else runs unchanged over the n-block maps.
// refine_image_stats_kernel, once behind the judge and once at the end, sums the maps per image (only when the caller asks).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "../../include/itw_dispatch.h"
#include "../../include/itw_decode.h"
#include "../../include/itw_amd.h"
#include "decode_core.hpp"
#include "texel_rows.hpp"
#include "kernels.hpp"
#include "host_rt.hpp"
#include <vector>

static_assert(sizeof(itw_refine_stats) == 56, "itw_refine_stats layout");
static_assert(sizeof(itw_refine_target_stats) == 144, "itw_refine_target_stats layout");

namespace itw {

constexpr int REFINE_PACKED_BLOCKS = 256;                       // blocks per row of the packed surface

// what the kernels accumulate; refine_finish_kernel turns it into itw_refine_stats
struct RefineAcc {
    unsigned long long sse_first, worst_first;                  // judge: over every block
    unsigned long long worst_final;                             // judge: blocks off the list; commit: listed blocks, whichever encoding stays
    unsigned long long gained, replaced;                        // commit: sum of eA - eB over, and number of, the blocks that took B
    uint32_t listed, met;                                       // scan; refine_round_begin_kernel: the target is met (itwCompressImageRefinedTo)
};
static_assert(sizeof(RefineAcc) == 48, "refine_begin_kernel: one lane per dword");

// the error of the block `w` against the 4 x 4 texels at `p` (rows `stride` bytes apart): measure_kernel's per-block sum over the channels in `mask`.
// CROP: only texel (x, y) with x < pw and y < ph counts -- the part of a chain's block that lies inside its image; the loads stay whole rows
// (the packed surface holds the replicated padding), only the accumulation is masked.
template <int FMT, bool CROP>
__device__ __forceinline__ unsigned long long refine_block_error(const uint4 w, const uint8_t* p, int64_t stride, uint32_t mask, int pw, int ph)
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
                    e += (((mask >> c) & 1u) && (!CROP || (x < pw && y < ph))) ? (unsigned long long)df * df : 0ull;
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
                    e += (((mask >> c) & 1u) && (!CROP || (x < pw && y < ph))) ? df * df : 0u;
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

// FMT: BCN_BC7 or BCN_BC6H (bcn_format.hpp).  `blocks`: 16-B aligned.  CROP: `extents` holds (pw - 1) | (ph - 1) << 2 per block (chain.hip)
template <int FMT, bool CROP>
__global__ void __launch_bounds__(256)
refine_judge_kernel(const uint8_t* __restrict__ blocks, int32_t blocks_x, int32_t nblocks, const uint8_t* __restrict__ src, int64_t stride,
                    uint32_t mask, unsigned long long budget, unsigned long long* __restrict__ emap, uint8_t* __restrict__ tmap,
                    uint32_t* __restrict__ group_count, RefineAcc* __restrict__ acc, const uint8_t* __restrict__ extents)
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
        const int ex = CROP ? (int)extents[b] : 15;
        e = refine_block_error<FMT, CROP>(w, src + (int64_t)yy * 4 * stride + (int64_t)xx * 4 * PX, stride, mask, (ex & 3) + 1, (ex >> 2) + 1);
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

// one lane per listed block: B = refined[i] against slot i of the packed surface; the rule; the winner into blocks / emap / tmap.
// CROP: the block's extent is extents[list[i]], as the judge took it.
template <int FMT, bool CROP>
__global__ void __launch_bounds__(256)
refine_commit_kernel(const uint32_t* __restrict__ list, int32_t n, int32_t packed_bx, const uint8_t* __restrict__ packed, int64_t pitch,
                     const uint8_t* __restrict__ refined, uint32_t mask, uint8_t* __restrict__ blocks, unsigned long long* __restrict__ emap,
                     uint8_t* __restrict__ tmap, RefineAcc* __restrict__ acc, const uint8_t* __restrict__ extents)
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
        const int ex = CROP ? (int)extents[b] : 15;
        const unsigned long long eb = refine_block_error<FMT, CROP>(w, packed + (int64_t)prow * 4 * pitch + (int64_t)pcol * 4 * PX, pitch, mask,
                                                                    (ex & 3) + 1, (ex >> 2) + 1);
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

// ---- itwCompressImageChainRefined[To]: the seven fields per image of the chain ----

__global__ void __launch_bounds__(256) refine_image_begin_kernel(uint32_t* __restrict__ p, int32_t dwords)
{
    const int32_t i = (int32_t)blockIdx.x * 256 + threadIdx.x;
    if (i < dwords) p[i] = 0u;
}

// The judge's 256 blocks per workgroup over the maps; a lane finds its image by chain_gather_kernel's binary search.  FINAL = false, behind
// the judge: blocks, sse_first, worst_first from the error map.  FINAL = true, last: listed and replaced from the tier map, sse_final and
// worst_final from the error map.  A wave inside one image reduces by shuffles and its first lane issues one atomic per field; a wave that
// spans images leaves the atomics to its lanes.  Integer add and max only: the order of arrival cannot change a field.
template <bool FINAL>
__global__ void __launch_bounds__(256)
refine_image_stats_kernel(const ChainImage* __restrict__ images, int32_t nimg, const unsigned long long* __restrict__ emap,
                          const uint8_t* __restrict__ tmap, int32_t nblocks, itw_refine_stats* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int32_t b = (int32_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = b < nblocks;
    const unsigned long long who = __ballot(live);
    if (who == 0ull) return;                                    // (no barrier below)
    int img = 0;
    unsigned long long e = 0ull;
    uint32_t listed = 0u, won = 0u;
    if (live) {
        int lo = 0, hi = nimg - 1;                              // the last image whose first block is <= b
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (images[mid].first_block <= (int64_t)b) lo = mid; else hi = mid - 1;
        }
        img = lo;
        e = emap[b];
        if (FINAL) { const uint32_t t = tmap[b]; listed = t != 0u ? 1u : 0u; won = t == 2u ? 1u : 0u; }
    }
    const int img0 = __shfl(img, 0);                            // lane 0 is live wherever a lane of its wave is
    unsigned long long sum = e, mx = e;
    uint32_t cnt = 1u;
    bool issue = live;
    if (__ballot(live && img == img0) == who) {
        sum = wave_sum(e); mx = wave_max(e); listed = wave_sum(listed); won = wave_sum(won);
        cnt = (uint32_t)__popcll(who);
        issue = lane == 0;
    }
    if (!issue) return;
    itw_refine_stats* s = out + img;
    if (!FINAL) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&s->blocks), (unsigned long long)cnt);
        if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(&s->sse_first), sum);
        if (mx) atomicMax(reinterpret_cast<unsigned long long*>(&s->worst_first), mx);
    } else {
        if (listed) atomicAdd(reinterpret_cast<unsigned long long*>(&s->listed), (unsigned long long)listed);
        if (won) atomicAdd(reinterpret_cast<unsigned long long*>(&s->replaced), (unsigned long long)won);
        if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(&s->sse_final), sum);
        if (mx) atomicMax(reinterpret_cast<unsigned long long*>(&s->worst_final), mx);
    }
}

// ---- itwCompressImageRefinedTo: the budget is chosen on the device ----

// Digit width of the select.  Keys are below 2^22 for BC7 (64 * 255^2) and below 2^39 for BC6H (64 * 0xFFFF^2): 11 bits make that two
// passes and four (22 and 44 bits); 8 bits would need three and five, 16 bits a 256-KiB histogram per pass that no workgroup keeps in LDS.
constexpr int SELECT_BITS = 11, SELECT_BINS = 1 << SELECT_BITS;
constexpr int SELECT_MAX_PASSES = 4;
constexpr int SELECT_PER_LANE = 8;                              // blocks per lane of select_hist_kernel: 2048 per workgroup
constexpr int REFINE_MAX_ROUNDS = 5;
__host__ __device__ constexpr int select_passes(int fmt) { return fmt == BCN_BC6H ? 4 : 2; }

struct RefineSelect {
    unsigned long long prefix, rank;                            // the digits chosen so far; the rank left among the candidates that share them
    unsigned long long budget[REFINE_MAX_ROUNDS];               // T of each round
    uint32_t done, _pad;                                        // at most k candidates: T = 0, the remaining passes return at once
};

struct RefineRounds { uint64_t listed[REFINE_MAX_ROUNDS]; uint64_t total_listed, target; uint32_t rounds; };

// 32 workgroups: clears hist[SELECT_MAX_PASSES][SELECT_BINS]; lane 0 of the first one starts round `round` with rank k.  check != 0: a
// stream whose summed error is already <= target sets acc->met instead, which turns the rest of the round into no-ops.
__global__ void __launch_bounds__(256)
refine_round_begin_kernel(RefineAcc* __restrict__ acc, RefineSelect* __restrict__ sel, uint32_t* __restrict__ hist, int32_t round,
                          unsigned long long k, unsigned long long target, int32_t check)
{
    const int32_t i = (int32_t)blockIdx.x * 256 + threadIdx.x;
    if (i < SELECT_MAX_PASSES * SELECT_BINS) hist[i] = 0u;
    if (i != 0) return;
    sel->prefix = 0ull; sel->rank = k; sel->done = 0u;
    if (round == 0) for (int j = 0; j < REFINE_MAX_ROUNDS; j++) sel->budget[j] = 0ull;
    const bool met = check && acc->sse_first - acc->gained <= target;
    acc->met = met ? 1u : 0u;
    if (!met && round == 0) acc->worst_final = 0ull;            // the judge's "everything stays"; from here on the commits' maximum
}

// pass over the digit at `shift`: hist[d] += candidates (tier 0, digits above the pass equal to sel->prefix) whose digit is d
__global__ void __launch_bounds__(256)
select_hist_kernel(const unsigned long long* __restrict__ emap, const uint8_t* __restrict__ tmap, int32_t nblocks, int32_t shift,
                   const RefineAcc* __restrict__ acc, const RefineSelect* __restrict__ sel, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t s_hist[SELECT_BINS];
    if (acc->met || sel->done || (acc->worst_first >> shift) == 0ull) return;
    const int t = threadIdx.x, lane = t & 63;
    for (int i = t; i < SELECT_BINS; i += 256) s_hist[i] = 0u;
    __syncthreads();
    const unsigned long long prefix = sel->prefix;
    const int32_t base = (int32_t)blockIdx.x * (256 * SELECT_PER_LANE);
#pragma unroll
    for (int i = 0; i < SELECT_PER_LANE; i++) {
        const int32_t b = base + i * 256 + t;
        bool cand = b < nblocks && tmap[b] == 0;
        const unsigned long long e = cand ? emap[b] : 0ull;
        cand = cand && ((e ^ prefix) >> (shift + SELECT_BITS)) == 0ull;
        const uint32_t d = (uint32_t)(e >> shift) & (uint32_t)(SELECT_BINS - 1);
        // one atomic for the wave where its candidates agree on the digit (the upper digits of most maps; flat content in any digit)
        const unsigned long long who = __ballot(cand);
        if (who == 0ull) continue;
        const uint32_t d0 = (uint32_t)__shfl((int)d, __ffsll((long long)who) - 1);
        if (__ballot(cand && d == d0) == who) {
            if (lane == 0) atomicAdd(&s_hist[d0], (uint32_t)__popcll(who));
        } else if (cand) {
            atomicAdd(&s_hist[d], 1u);
        }
    }
    __syncthreads();
    for (int i = t; i < SELECT_BINS; i += 256) { const uint32_t v = s_hist[i]; if (v) atomicAdd(&hist[i], v); }
}

// ONE workgroup, 8 bins per lane from the top bin down: the digit d with #(digits above d) <= rank < #(digits >= d) joins the prefix, and
// the rank becomes the rank within d.  rank >= the candidates counted: there are at most k of them, T stays 0.  last: T = the prefix.
__global__ void __launch_bounds__(256)
select_scan_kernel(const uint32_t* __restrict__ hist, int32_t shift, int32_t last, int32_t round, const RefineAcc* __restrict__ acc,
                   RefineSelect* __restrict__ sel)
{
    constexpr int PER = SELECT_BINS / 256;
    __shared__ unsigned long long s_wave[4];
    if (acc->met || sel->done || (acc->worst_first >> shift) == 0ull) return;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const unsigned long long rank = sel->rank, prefix = sel->prefix;
    uint32_t v[PER];
    unsigned long long sum = 0ull;
#pragma unroll
    for (int j = 0; j < PER; j++) { v[j] = hist[SELECT_BINS - 1 - (t * PER + j)]; sum += v[j]; }
    unsigned long long inc = sum;                               // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long u = __shfl_up(inc, o); if (lane >= o) inc += u; }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();                                            // (also: every lane has read sel before one of them writes it)
    unsigned long long before = 0ull, total = 0ull;
#pragma unroll
    for (int k = 0; k < 4; k++) { const unsigned long long wv = s_wave[k]; before += k < wave ? wv : 0ull; total += wv; }
    if (rank >= total) { if (t == 0) sel->done = 1u; return; }
    unsigned long long above = before + inc - sum;              // candidates in the bins above this lane's first
#pragma unroll
    for (int j = 0; j < PER; j++) {
        if (above <= rank && rank < above + v[j]) {
            const unsigned long long p = prefix | ((unsigned long long)(SELECT_BINS - 1 - (t * PER + j)) << shift);
            sel->prefix = p; sel->rank = rank - above;
            if (last) sel->budget[round] = p;
        }
        above += v[j];
    }
}

// The judge's 256 blocks per workgroup over the maps it left: listed = still at tier 0 and above *budget; the workgroup's count.  The judge's
// other job with a host-known budget, the largest error among the blocks that stay, needs no pass here: of the candidates that stay the
// largest is T itself (T is a candidate's error, or 0 when every inexact candidate is listed), and the blocks refined in earlier rounds
// are in acc->worst_final from their commits -- refine_finish_to_kernel puts the two together.  (Measured at 4096^2: one atomic maximum per
// workgroup on that one word made this kernel 49 us, against 4 us for the loads; the judge hides the same atomics behind its decode.)
__global__ void __launch_bounds__(256)
refine_count_kernel(const unsigned long long* __restrict__ emap, const uint8_t* __restrict__ tmap, int32_t nblocks,
                    const unsigned long long* __restrict__ budget, uint32_t* __restrict__ group_count, const RefineAcc* __restrict__ acc)
{
    __shared__ uint32_t s_cnt[4];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    if (acc->met) { if (t == 0) group_count[blockIdx.x] = 0u; return; }
    const int32_t b = (int32_t)blockIdx.x * 256 + t;
    const bool listed = b < nblocks && tmap[b] == 0 && emap[b] > *budget;
    const uint32_t cnt = (uint32_t)__popcll(__ballot(listed));
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (t == 0) group_count[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// refine_list_kernel with the budget behind a pointer and the tier filter
__global__ void __launch_bounds__(256)
refine_list_to_kernel(const unsigned long long* __restrict__ emap, const uint8_t* __restrict__ tmap, int32_t nblocks,
                      const unsigned long long* __restrict__ budget, const uint32_t* __restrict__ group_first, uint32_t* __restrict__ list)
{
    __shared__ uint32_t s_cnt[4];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int32_t b = (int32_t)blockIdx.x * 256 + t;
    const bool listed = b < nblocks && tmap[b] == 0 && emap[b] > *budget;
    const unsigned long long ballot = __ballot(listed);
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t before = 0u;
#pragma unroll
    for (int k = 0; k < 3; k++) before += k < wave ? s_cnt[k] : 0u;
    if (listed) list[group_first[blockIdx.x] + before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull))] = (uint32_t)b;
}

__global__ void refine_finish_to_kernel(const RefineAcc* __restrict__ acc, const RefineSelect* __restrict__ sel, unsigned long long nblocks,
                                        RefineRounds r, itw_refine_target_stats* __restrict__ stats)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long sse_final = acc->sse_first - acc->gained;
    stats->total.blocks = nblocks;
    stats->total.listed = r.total_listed;
    stats->total.replaced = acc->replaced;
    stats->total.sse_first = acc->sse_first;
    stats->total.sse_final = sse_final;
    stats->total.worst_first = acc->worst_first;
    // the blocks refined in any round, and the candidates that stayed in the last one: the largest of those is its T
    const unsigned long long stay = r.rounds ? sel->budget[r.rounds - 1] : 0ull;
    stats->total.worst_final = acc->worst_final > stay ? acc->worst_final : stay;
    stats->rounds = r.rounds;
    stats->target_met = sse_final <= r.target ? 1u : 0u;
    for (uint32_t j = 0; j < (uint32_t)REFINE_MAX_ROUNDS; j++) {
        stats->budget[j] = j < r.rounds ? sel->budget[j] : 0ull;
        stats->listed[j] = r.listed[j];
    }
}

} // namespace itw

namespace {

// offsets into a scratch buffer, each a multiple of 256
struct Carve {
    size_t used = 0;
    size_t take(size_t bytes) { const size_t at = used; used += (bytes + 255) & ~(size_t)255; return at; }
};

// What the core reads its texels from: block b of the call lies at block row b / blocks_x, column b % blocks_x of a device surface whose
// rows are `stride` bytes apart.  `extents` (optional): per block, the part of it that lies inside its image (chain.hip); `images` /
// `nimg` (a chain only): the device table the per-image kernel searches.
struct RefineView { const uint8_t* src; int64_t stride; int32_t blocks_x; const uint8_t* extents; const itw::ChainImage* images; int32_t nimg; };

// The two front doors.  Each knows, before any device work, how many blocks the call judges (nb), the surface its first tier encodes
// (bx x by blocks: a chain's last packed row may run past nb) and how much of scratch 0 it wants; prepare() queues whatever makes the
// texels device-resident and returns the view.
struct Front {
    int64_t nb = 0;
    int32_t bx = 0, by = 0;
    size_t bytes = 0;
    int nimg = 0;                                               // images a caller may ask per-image stats for (a chain)
    bool packed = false;                                        // the first tier writes bx * by >= nb blocks: never straight into the target
    virtual RefineView prepare(uint8_t* scratch, hipStream_t st) = 0;
    virtual ~Front() = default;
};

// one surface, read in place (a host surface: from its staged copy)
struct SurfaceFront final : Front {
    const rgba_surface& s;
    bool dsrc;
    size_t row_bytes, pitch;
    SurfaceFront(int kind, const rgba_surface& surface) : s(surface)
    {
        bx = s.width / 4; by = s.height / 4; nb = (int64_t)bx * by;
        dsrc = itw::is_device_pointer(s.ptr);
        row_bytes = (size_t)s.width * itw::texel_bytes(kind); pitch = (row_bytes + 15) & ~(size_t)15;
        bytes = dsrc ? 0 : pitch * (size_t)s.height;
    }
    RefineView prepare(uint8_t* scratch, hipStream_t st) override
    {
        if (dsrc) return RefineView{s.ptr, (int64_t)s.stride, bx, nullptr, nullptr, 0};
        ITW_CHECK(hipMemcpy2DAsync(scratch, pitch, s.ptr, (size_t)s.stride, row_bytes, (size_t)s.height, hipMemcpyHostToDevice, st));
        return RefineView{scratch, (int64_t)pitch, bx, nullptr, nullptr, 0};
    }
};

// a chain: every image gathered, with edge replication, into ONE packed surface of min(1024, nb) blocks per row (chain.hip) -- the chain
// is one population of blocks, so that the lists, the select and the refine tier see all of it at once
struct ChainFront final : Front {
    const rgba_surface* im;
    int count, px;
    bool dsrc;
    int64_t pitch;
    size_t o_table, o_extents, o_packed;
    std::vector<size_t> o_stage;
    std::vector<itw::ChainImage> desc;                          // lives until the call has synchronised
    ChainFront(const char* who, int kind, const rgba_surface* images, int n) : im(images), count(n), px(itw::texel_bytes(kind))
    {
        packed = true; nimg = n;
        dsrc = itw::all_one_pointer_kind(who, "image", im, count);
        if (dsrc) {
            int cur = 0;
            ITW_CHECK(hipGetDevice(&cur));
            for (int i = 0; i < count; i++) {
                hipPointerAttribute_t a = {};
                ITW_CHECK(hipPointerGetAttributes(&a, im[i].ptr));
                if (a.type == hipMemoryTypeDevice && a.device != cur)
                    itw::fail_msg("%s: image %d lives on device %d, the calling thread's current device is %d", who, i, a.device, cur);
            }
        }
        for (int i = 0; i < count; i++) nb += itw::image_blocks(im[i]);
        bx = (int32_t)(nb < 1024 ? nb : 1024); by = (int32_t)((nb + bx - 1) / bx);
        pitch = (int64_t)bx * 4 * px;
        Carve c;
        o_table = c.take((size_t)count * sizeof(itw::ChainImage));
        o_extents = c.take((size_t)nb);
        o_packed = c.take((size_t)pitch * 4 * (size_t)by);
        if (!dsrc) {
            o_stage.resize((size_t)count);
            for (int i = 0; i < count; i++) o_stage[(size_t)i] = c.take((((size_t)im[i].width * px + 15) & ~(size_t)15) * (size_t)im[i].height);
        }
        bytes = c.used;
    }
    RefineView prepare(uint8_t* scratch, hipStream_t st) override
    {
        desc.resize((size_t)count);
        int64_t first = 0;
        for (int i = 0; i < count; i++) {
            itw::ChainImage& d = desc[(size_t)i];
            const size_t row_bytes = (size_t)im[i].width * px, row_pitch = (row_bytes + 15) & ~(size_t)15;
            if (!dsrc) ITW_CHECK(hipMemcpy2DAsync(scratch + o_stage[(size_t)i], row_pitch, im[i].ptr, (size_t)im[i].stride, row_bytes, (size_t)im[i].height,
                                                  hipMemcpyHostToDevice, st));
            d.ptr = dsrc ? im[i].ptr : scratch + o_stage[(size_t)i];
            d.stride = dsrc ? (int64_t)im[i].stride : (int64_t)row_pitch;
            d.width = im[i].width; d.height = im[i].height;
            d.first_block = first;
            first += itw::image_blocks(im[i]);
        }
        itw::ChainImage* table = reinterpret_cast<itw::ChainImage*>(scratch + o_table);
        ITW_CHECK(hipMemcpyAsync(table, desc.data(), desc.size() * sizeof(itw::ChainImage), hipMemcpyHostToDevice, st));
        itw::launch_chain_gather(table, count, nb, bx, by, px, false, scratch + o_packed, pitch, st, scratch + o_extents);
        return RefineView{scratch + o_packed, pitch, bx, scratch + o_extents, table, count};
    }
};

struct Outputs { uint8_t* target; void* stats; size_t stats_size; itw_refine_stats* image_stats; uint64_t* block_sse; uint8_t* tier_map; };

// The core both calls and both front doors share: scratch, the first tier, the judge; one refine tier over a list; the way out.
// Everything that needs the device.
struct Call {
    hipStream_t st;
    int kind, px, dxgi_format;
    const void* second;
    uint32_t mask;
    int64_t nb;
    int32_t groups;
    Outputs out;
    bool dtgt, dstats, dmap, dtier, dimage;
    RefineView v;
    itw::RefineAcc* acc;
    void* d_stats;
    itw::RefineSelect* sel;
    uint32_t *hist, *group_count, *group_first, *list, *host_n;
    uint8_t *d_tgt, *d_tier, *front_scratch;
    unsigned long long* d_map;
    itw_refine_stats* d_image;
    bool done = false;

    Call(const Call&) = delete;
    Call& operator=(const Call&) = delete;
    // a failure is a C++ exception: what the call has queued by then is drained, so that the next call finds the scratch idle
    ~Call() { if (!done) { (void)hipStreamSynchronize(st); (void)hipGetLastError(); } }

    // `select`: room for the select's state (itwCompressImageRefinedTo).  Carves the scratch; queues nothing (a constructor that throws
    // runs no destructor: the work starts in open())
    Call(int kind_, Front& f, const Outputs& o, int dxgi_format_, const void* second_, uint32_t mask_, bool select)
        : st((hipStream_t)itwGetStream()), kind(kind_), px(itw::texel_bytes(kind_)), dxgi_format(dxgi_format_), second(second_), mask(mask_), nb(f.nb),
          groups((int32_t)((f.nb + 255) / 256)), out(o)
    {
        using namespace itw;
        // the kernels take device memory; the judge and the commit load and store whole blocks as 16-B vectors
        dtgt = !f.packed && is_device_pointer(out.target) && ((uintptr_t)out.target & 15) == 0;
        dstats = is_device_pointer(out.stats);
        dmap = out.block_sse && is_device_pointer(out.block_sse);
        dtier = out.tier_map && is_device_pointer(out.tier_map);
        dimage = out.image_stats && is_device_pointer(out.image_stats);
        Carve c0;
        const size_t o_acc = c0.take(sizeof(RefineAcc)), o_stats = c0.take(out.stats_size), o_sel = c0.take(select ? sizeof(RefineSelect) : 0),
                     o_hist = c0.take(select ? (size_t)SELECT_MAX_PASSES * SELECT_BINS * 4 : 0), o_count = c0.take((size_t)groups * 4),
                     o_first = c0.take((size_t)groups * 4), o_list = c0.take((size_t)nb * 4), o_front = c0.take(f.bytes),
                     o_tgt = c0.take(dtgt ? 0 : (size_t)f.bx * f.by * 16), o_map = c0.take(dmap ? 0 : (size_t)nb * 8), o_tier = c0.take(dtier ? 0 : (size_t)nb),
                     o_image = c0.take(out.image_stats && !dimage ? sizeof(itw_refine_stats) * (size_t)f.nimg : 0);
        uint8_t* base = static_cast<uint8_t*>(refine_scratch(0, c0.used));
        acc = reinterpret_cast<RefineAcc*>(base + o_acc);
        d_stats = dstats ? out.stats : base + o_stats;
        sel = reinterpret_cast<RefineSelect*>(base + o_sel);
        hist = reinterpret_cast<uint32_t*>(base + o_hist);
        group_count = reinterpret_cast<uint32_t*>(base + o_count);
        group_first = reinterpret_cast<uint32_t*>(base + o_first);
        list = reinterpret_cast<uint32_t*>(base + o_list);
        d_tgt = dtgt ? out.target : base + o_tgt;
        d_map = reinterpret_cast<unsigned long long*>(dmap ? reinterpret_cast<uint8_t*>(out.block_sse) : base + o_map);
        d_tier = dtier ? out.tier_map : base + o_tier;
        d_image = dimage ? out.image_stats : reinterpret_cast<itw_refine_stats*>(base + o_image);
        host_n = refine_count_word();                           // [0] acc->listed, [1] acc->met
        front_scratch = base + o_front;
    }

    // queues the texels, the first tier and the judge with `budget`
    void open(Front& f, const void* first, unsigned long long budget)
    {
        using namespace itw;
        v = f.prepare(front_scratch, st);
        encode_resident(dxgi_format, first, v.src, v.stride, f.bx * 4, f.by * 4, d_tgt);

        const dim3 grid((unsigned)groups), blk(256);
        hipLaunchKernelGGL(refine_begin_kernel, dim3(1), dim3(64), 0, st, acc);
        ITW_CHECK(hipGetLastError());
        if (v.extents) {
            if (kind == BCN_BC7) hipLaunchKernelGGL((refine_judge_kernel<BCN_BC7, true>), grid, blk, 0, st, d_tgt, v.blocks_x, (int32_t)nb, v.src, v.stride, mask,
                                                    budget, d_map, d_tier, group_count, acc, v.extents);
            else                 hipLaunchKernelGGL((refine_judge_kernel<BCN_BC6H, true>), grid, blk, 0, st, d_tgt, v.blocks_x, (int32_t)nb, v.src, v.stride, mask,
                                                    budget, d_map, d_tier, group_count, acc, v.extents);
        } else {
            if (kind == BCN_BC7) hipLaunchKernelGGL((refine_judge_kernel<BCN_BC7, false>), grid, blk, 0, st, d_tgt, v.blocks_x, (int32_t)nb, v.src, v.stride, mask,
                                                    budget, d_map, d_tier, group_count, acc, v.extents);
            else                 hipLaunchKernelGGL((refine_judge_kernel<BCN_BC6H, false>), grid, blk, 0, st, d_tgt, v.blocks_x, (int32_t)nb, v.src, v.stride, mask,
                                                    budget, d_map, d_tier, group_count, acc, v.extents);
        }
        ITW_CHECK(hipGetLastError());
        if (out.image_stats) {
            const int32_t dwords = (int32_t)(sizeof(itw_refine_stats) / 4) * v.nimg;
            hipLaunchKernelGGL(refine_image_begin_kernel, dim3((unsigned)((dwords + 255) / 256)), blk, 0, st, reinterpret_cast<uint32_t*>(d_image), dwords);
            ITW_CHECK(hipGetLastError());
            hipLaunchKernelGGL((refine_image_stats_kernel<false>), grid, blk, 0, st, v.images, v.nimg, d_map, d_tier, (int32_t)nb, d_image);
            ITW_CHECK(hipGetLastError());
        }
    }

    // the refine tier over list[0, n), n > 0, which the caller's list kernel has queued: gather, encode, commit
    void refine_listed(int64_t n)
    {
        using namespace itw;
        const int32_t pbx = (int32_t)(n < REFINE_PACKED_BLOCKS ? n : REFINE_PACKED_BLOCKS), pby = (int32_t)((n + pbx - 1) / pbx);
        const int32_t total = pbx * pby;
        const int64_t pitch = (int64_t)pbx * 4 * px;
        Carve c1;
        const size_t o_packed = c1.take((size_t)pitch * 4 * pby), o_refined = c1.take((size_t)total * 16);
        uint8_t* lbase = static_cast<uint8_t*>(refine_scratch(1, c1.used));
        uint8_t* packed = lbase + o_packed;
        uint8_t* refined = lbase + o_refined;
        const dim3 blk(256), ggrid((unsigned)((total + 63) / 64)), cgrid((unsigned)((n + 255) / 256));
        if (kind == BCN_BC7) hipLaunchKernelGGL((refine_gather_kernel<4>), ggrid, blk, 0, st, list, (int32_t)n, total, pbx, v.src, v.stride, v.blocks_x, packed, pitch);
        else                 hipLaunchKernelGGL((refine_gather_kernel<8>), ggrid, blk, 0, st, list, (int32_t)n, total, pbx, v.src, v.stride, v.blocks_x, packed, pitch);
        ITW_CHECK(hipGetLastError());
        encode_resident(dxgi_format, second, packed, pitch, pbx * 4, pby * 4, refined);
        if (v.extents) {
            if (kind == BCN_BC7) hipLaunchKernelGGL((refine_commit_kernel<BCN_BC7, true>), cgrid, blk, 0, st, list, (int32_t)n, pbx, packed, pitch, refined, mask, d_tgt, d_map, d_tier, acc, v.extents);
            else                 hipLaunchKernelGGL((refine_commit_kernel<BCN_BC6H, true>), cgrid, blk, 0, st, list, (int32_t)n, pbx, packed, pitch, refined, mask, d_tgt, d_map, d_tier, acc, v.extents);
        } else {
            if (kind == BCN_BC7) hipLaunchKernelGGL((refine_commit_kernel<BCN_BC7, false>), cgrid, blk, 0, st, list, (int32_t)n, pbx, packed, pitch, refined, mask, d_tgt, d_map, d_tier, acc, v.extents);
            else                 hipLaunchKernelGGL((refine_commit_kernel<BCN_BC6H, false>), cgrid, blk, 0, st, list, (int32_t)n, pbx, packed, pitch, refined, mask, d_tgt, d_map, d_tier, acc, v.extents);
        }
        ITW_CHECK(hipGetLastError());
    }

    // behind the caller's finish kernel: the per-image fields of the stream written, then whatever the caller did not pass device memory for
    void close()
    {
        using namespace itw;
        if (out.image_stats) {
            hipLaunchKernelGGL((refine_image_stats_kernel<true>), dim3((unsigned)groups), dim3(256), 0, st, v.images, v.nimg, d_map, d_tier, (int32_t)nb, d_image);
            ITW_CHECK(hipGetLastError());
        }
        if (!dtgt) ITW_CHECK(hipMemcpyAsync(out.target, d_tgt, (size_t)nb * 16, hipMemcpyDefault, st));
        if (!dstats) ITW_CHECK(hipMemcpyAsync(out.stats, d_stats, out.stats_size, hipMemcpyDeviceToHost, st));
        if (out.image_stats && !dimage) ITW_CHECK(hipMemcpyAsync(out.image_stats, d_image, sizeof(itw_refine_stats) * (size_t)v.nimg, hipMemcpyDeviceToHost, st));
        if (out.block_sse && !dmap) ITW_CHECK(hipMemcpyAsync(out.block_sse, d_map, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
        if (out.tier_map && !dtier) ITW_CHECK(hipMemcpyAsync(out.tier_map, d_tier, (size_t)nb, hipMemcpyDeviceToHost, st));
        ITW_CHECK(hipStreamSynchronize(st));
        done = true;
    }
};

void refine(const char* who, int kind, Front& f, const Outputs& out, int dxgi_format, const void* first, const void* second, uint32_t mask, uint64_t budget)
{
    using namespace itw;
    Call c(kind, f, out, dxgi_format, second, mask, false);
    c.open(f, first, (unsigned long long)budget);
    const dim3 blk(256);
    hipLaunchKernelGGL(refine_scan_kernel, dim3(1), blk, 0, c.st, c.group_count, c.groups, c.group_first, c.acc);
    ITW_CHECK(hipGetLastError());
    ITW_CHECK(hipMemcpyAsync(c.host_n, &c.acc->listed, sizeof(uint32_t), hipMemcpyDeviceToHost, c.st));
    ITW_CHECK(hipStreamSynchronize(c.st));
    const int64_t n = (int64_t)*c.host_n;
    if (n < 0 || n > c.nb) fail_msg("%s: %lld blocks listed of %lld", who, (long long)n, (long long)c.nb);
    if (n > 0) {
        hipLaunchKernelGGL(refine_list_kernel, dim3((unsigned)c.groups), blk, 0, c.st, c.d_map, (int32_t)c.nb, (unsigned long long)budget, c.group_first, c.list);
        ITW_CHECK(hipGetLastError());
        c.refine_listed(n);
    }
    hipLaunchKernelGGL(refine_finish_kernel, dim3(1), dim3(64), 0, c.st, c.acc, (unsigned long long)c.nb, static_cast<itw_refine_stats*>(c.d_stats));
    ITW_CHECK(hipGetLastError());
    c.close();
}

// itwCompressImage[Chain]RefinedTo: refine() with the budget of every round chosen on the device
void refine_to(const char* who, int kind, Front& f, const Outputs& out, int dxgi_format, const void* first, const void* second, uint32_t mask,
               const itw_refine_policy& policy)
{
    using namespace itw;
    // the judge with a budget that lists nothing: the maps, sse_first, worst_first, and worst_final for a call that runs no round
    Call c(kind, f, out, dxgi_format, second, mask, true);
    c.open(f, first, ~0ull);
    hipStream_t st = c.st;
    const int64_t nb = c.nb;
    const int32_t groups = c.groups;
    RefineAcc* acc = c.acc;
    RefineSelect* sel = c.sel;
    uint32_t* host_n = c.host_n;
    const dim3 blk(256);

    const bool single = policy.target_total_sse == UINT64_MAX;  // policy A
    const int passes = select_passes(kind);
    const dim3 hgrid((unsigned)((nb + 256 * SELECT_PER_LANE - 1) / (256 * SELECT_PER_LANE)));
    RefineRounds r = {};
    r.target = policy.target_total_sse;
    uint64_t cap_left = policy.max_listed;
    for (int j = 0; j < (single ? 1 : REFINE_MAX_ROUNDS); j++) {
        if (!single && cap_left == 0) break;
        const uint64_t q = j < 4 ? (uint64_t)((nb >> (4 - j)) > 0 ? (nb >> (4 - j)) : 1) : (uint64_t)nb;
        const uint64_t k = single ? policy.max_listed : (cap_left < q ? cap_left : q);
        // the whole round up to its list length goes on the stream at once; what it does is decided by device words
        hipLaunchKernelGGL(refine_round_begin_kernel, dim3(SELECT_MAX_PASSES * SELECT_BINS / 256), blk, 0, st, acc, sel, c.hist, (int32_t)j,
                           (unsigned long long)k, (unsigned long long)policy.target_total_sse, (int32_t)(single ? 0 : 1));
        ITW_CHECK(hipGetLastError());
        for (int p = passes - 1; p >= 0; p--) {
            hipLaunchKernelGGL(select_hist_kernel, hgrid, blk, 0, st, c.d_map, c.d_tier, (int32_t)nb, (int32_t)(p * SELECT_BITS), acc, sel, c.hist + p * SELECT_BINS);
            ITW_CHECK(hipGetLastError());
            hipLaunchKernelGGL(select_scan_kernel, dim3(1), blk, 0, st, c.hist + p * SELECT_BINS, (int32_t)(p * SELECT_BITS), (int32_t)(p == 0), (int32_t)j, acc, sel);
            ITW_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(refine_count_kernel, dim3((unsigned)groups), blk, 0, st, c.d_map, c.d_tier, (int32_t)nb, &sel->budget[j], c.group_count, acc);
        ITW_CHECK(hipGetLastError());
        hipLaunchKernelGGL(refine_scan_kernel, dim3(1), blk, 0, st, c.group_count, groups, c.group_first, acc);
        ITW_CHECK(hipGetLastError());
        ITW_CHECK(hipMemcpyAsync(host_n, &acc->listed, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        ITW_CHECK(hipStreamSynchronize(st));
        if (host_n[1]) break;                                   // the target was met before this round: it ran nothing
        const int64_t n = (int64_t)host_n[0];
        if (n < 0 || n > nb || (uint64_t)n > k) fail_msg("%s: %lld blocks listed of %lld, rank %llu", who, (long long)n, (long long)nb, (unsigned long long)k);
        r.rounds = (uint32_t)j + 1u;
        r.listed[j] = (uint64_t)n;
        r.total_listed += (uint64_t)n;
        if (cap_left != UINT64_MAX) cap_left -= (uint64_t)n;
        if (n == 0) continue;
        hipLaunchKernelGGL(refine_list_to_kernel, dim3((unsigned)groups), blk, 0, st, c.d_map, c.d_tier, (int32_t)nb, &sel->budget[j], c.group_first, c.list);
        ITW_CHECK(hipGetLastError());
        c.refine_listed(n);
    }
    hipLaunchKernelGGL(refine_finish_to_kernel, dim3(1), dim3(64), 0, st, acc, sel, (unsigned long long)nb, r, static_cast<itw_refine_target_stats*>(c.d_stats));
    ITW_CHECK(hipGetLastError());
    c.close();
}

// the checks both entries share, none of which needs a device; returns the block kind
int check_refined_call(const char* who, const rgba_surface* source, const uint8_t* target, int dxgi_format, const void* first_settings,
                       const void* refine_settings, uint32_t channel_mask, const void* stats, size_t stats_bytes, size_t stats_size,
                       const char* stats_type, const uint64_t* block_sse)
{
    itw::refuse_signed_bc6h(who, dxgi_format);
    const int kind = itw::format_kind(dxgi_format);
    if (kind != itw::BCN_BC7 && kind != itw::BCN_BC6H) itw::fail_msg("%s: DXGI format %d has one encoder only (BC7 and BC6H have presets to refine with)", who, dxgi_format);
    if (!source || !source->ptr || !target) itw::fail_msg("%s: null surface, texel or target pointer", who);
    if (!first_settings || !refine_settings) itw::fail_msg("%s: null settings for the %s tier", who, first_settings ? "refine" : "first");
    if (!stats) itw::fail_msg("%s: null stats", who);
    if (stats_bytes != stats_size) itw::fail_msg("%s: stats_bytes %zu != sizeof(%s) = %zu", who, stats_bytes, stats_type, stats_size);
    if (((uintptr_t)stats & 7) || ((uintptr_t)block_sse & 7)) itw::fail_msg("%s: stats and block_sse must be 8-byte aligned", who);
    if (channel_mask == 0 || channel_mask > 15) itw::fail_msg("%s: channel mask %u (1..15: bit 0 = R .. bit 3 = A)", who, channel_mask);
    if (source->width < 4 || source->height < 4 || (source->width & 3) || (source->height & 3))
        itw::fail_msg("%s: %d x %d: width and height must be multiples of 4 (itwPadToMultipleOf4)", who, source->width, source->height);
    const int64_t row = (int64_t)source->width * itw::texel_bytes(kind);
    if ((int64_t)source->stride < row) itw::fail_msg("%s: stride %d < %lld bytes per row", who, source->stride, (long long)row);
    if ((int64_t)(source->width / 4) * (source->height / 4) > (int64_t)ITW_MEASURE_MAX_BLOCKS)
        itw::fail_msg("%s: %d x %d is more than %lld blocks", who, source->width, source->height, (long long)ITW_MEASURE_MAX_BLOCKS);
    return kind;
}

// the same for a chain: the refined calls' checks, then itwCompressImageChainEx's, then the chain's block count; returns the block kind
int check_refined_chain_call(const char* who, const rgba_surface* images, int count, const uint8_t* target, int dxgi_format, const void* first_settings,
                             const void* refine_settings, uint32_t channel_mask, const void* stats, size_t stats_bytes, size_t stats_size,
                             const char* stats_type, const itw_refine_stats* image_stats, const uint64_t* block_sse)
{
    itw::refuse_signed_bc6h(who, dxgi_format);
    const int kind = itw::format_kind(dxgi_format);
    if (kind != itw::BCN_BC7 && kind != itw::BCN_BC6H) itw::fail_msg("%s: DXGI format %d has one encoder only (BC7 and BC6H have presets to refine with)", who, dxgi_format);
    if (!first_settings || !refine_settings) itw::fail_msg("%s: null settings for the %s tier", who, first_settings ? "refine" : "first");
    itw::chain_check(images, count, target, dxgi_format);       // count, null pointers, sizes, strides
    if (!stats) itw::fail_msg("%s: null stats", who);
    if (stats_bytes != stats_size) itw::fail_msg("%s: stats_bytes %zu != sizeof(%s) = %zu", who, stats_bytes, stats_type, stats_size);
    if (((uintptr_t)stats & 7) || ((uintptr_t)image_stats & 7) || ((uintptr_t)block_sse & 7))
        itw::fail_msg("%s: stats, image_stats and block_sse must be 8-byte aligned", who);
    if (channel_mask == 0 || channel_mask > 15) itw::fail_msg("%s: channel mask %u (1..15: bit 0 = R .. bit 3 = A)", who, channel_mask);
    int64_t total = 0;
    for (int i = 0; i < count; i++) {
        total += itw::image_blocks(images[i]);
        if (total > (int64_t)ITW_MEASURE_MAX_BLOCKS)
            itw::fail_msg("%s: images 0 .. %d are more than %lld blocks", who, i, (long long)ITW_MEASURE_MAX_BLOCKS);
    }
    return kind;
}

// itwPsnrToTotalSse over n = texels x selected channels
uint64_t psnr_to_total_sse(int dxgi_format, double texels, uint32_t channel_mask, double psnr_db)
{
    const int kind = itw::format_kind(dxgi_format);
    int channels = 0;
    for (int c = 0; c < 4; c++) channels += (channel_mask >> c) & 1u;
    if (kind == itw::BCN_NONE || kind == itw::BCN_BC6H || kind == itw::BCN_ETC1 || channels == 0 || !(texels >= 1.0) || !std::isfinite(psnr_db)) return UINT64_MAX;
    const double peak = (kind == itw::BCN_BC4S || kind == itw::BCN_BC5S) ? 254.0 : 255.0;      // as itwStatsPsnr
    const double sse = std::floor(peak * peak * (texels * (double)channels) / std::pow(10.0, psnr_db / 10.0));
    return sse >= 18446744073709551615.0 ? UINT64_MAX : (uint64_t)sse;
}

} // namespace

extern "C" bool itwCompressImageRefined(const rgba_surface* source, uint8_t* target, int dxgi_format, const void* first_settings,
                                        const void* refine_settings, uint32_t channel_mask, uint64_t max_block_sse, itw_refine_stats* stats,
                                        size_t stats_bytes, uint64_t* block_sse, uint8_t* tier_map)
{
    itw::clear_failure();
    return itw::guarded([&] {
        const char* who = "itwCompressImageRefined";
        const int kind = check_refined_call(who, source, target, dxgi_format, first_settings, refine_settings, channel_mask, stats,
                                            stats_bytes, sizeof(itw_refine_stats), "itw_refine_stats", block_sse);
        SurfaceFront front(kind, *source);
        refine(who, kind, front, Outputs{target, stats, sizeof(itw_refine_stats), nullptr, block_sse, tier_map}, dxgi_format, first_settings,
               refine_settings, channel_mask, max_block_sse);
    });
}

extern "C" bool itwCompressImageRefinedTo(const rgba_surface* source, uint8_t* target, int dxgi_format, const void* first_settings,
                                          const void* refine_settings, uint32_t channel_mask, const itw_refine_policy* policy, size_t policy_bytes,
                                          itw_refine_target_stats* stats, size_t stats_bytes, uint64_t* block_sse, uint8_t* tier_map)
{
    itw::clear_failure();
    return itw::guarded([&] {
        const char* who = "itwCompressImageRefinedTo";
        if (!policy) itw::fail_msg("%s: null policy", who);
        if (policy_bytes != sizeof(itw_refine_policy))
            itw::fail_msg("%s: policy_bytes %zu != sizeof(itw_refine_policy) = %zu", who, policy_bytes, sizeof(itw_refine_policy));
        const int kind = check_refined_call(who, source, target, dxgi_format, first_settings, refine_settings, channel_mask, stats,
                                            stats_bytes, sizeof(itw_refine_target_stats), "itw_refine_target_stats", block_sse);
        SurfaceFront front(kind, *source);
        refine_to(who, kind, front, Outputs{target, stats, sizeof(itw_refine_target_stats), nullptr, block_sse, tier_map}, dxgi_format, first_settings,
                  refine_settings, channel_mask, *policy);
    });
}

extern "C" bool itwCompressImageChainRefined(const rgba_surface* images, int count, uint8_t* target, int dxgi_format, const void* first_settings,
                                             const void* refine_settings, uint32_t channel_mask, uint64_t max_block_sse, itw_refine_stats* stats,
                                             size_t stats_bytes, itw_refine_stats* image_stats, uint64_t* block_sse, uint8_t* tier_map)
{
    itw::clear_failure();
    return itw::guarded([&] {
        const char* who = "itwCompressImageChainRefined";
        const int kind = check_refined_chain_call(who, images, count, target, dxgi_format, first_settings, refine_settings, channel_mask, stats,
                                                  stats_bytes, sizeof(itw_refine_stats), "itw_refine_stats", image_stats, block_sse);
        ChainFront front(who, kind, images, count);
        refine(who, kind, front, Outputs{target, stats, sizeof(itw_refine_stats), image_stats, block_sse, tier_map}, dxgi_format, first_settings,
               refine_settings, channel_mask, max_block_sse);
    });
}

extern "C" bool itwCompressImageChainRefinedTo(const rgba_surface* images, int count, uint8_t* target, int dxgi_format, const void* first_settings,
                                               const void* refine_settings, uint32_t channel_mask, const itw_refine_policy* policy,
                                               size_t policy_bytes, itw_refine_target_stats* stats, size_t stats_bytes,
                                               itw_refine_stats* image_stats, uint64_t* block_sse, uint8_t* tier_map)
{
    itw::clear_failure();
    return itw::guarded([&] {
        const char* who = "itwCompressImageChainRefinedTo";
        if (!policy) itw::fail_msg("%s: null policy", who);
        if (policy_bytes != sizeof(itw_refine_policy))
            itw::fail_msg("%s: policy_bytes %zu != sizeof(itw_refine_policy) = %zu", who, policy_bytes, sizeof(itw_refine_policy));
        const int kind = check_refined_chain_call(who, images, count, target, dxgi_format, first_settings, refine_settings, channel_mask, stats,
                                                  stats_bytes, sizeof(itw_refine_target_stats), "itw_refine_target_stats", image_stats, block_sse);
        ChainFront front(who, kind, images, count);
        refine_to(who, kind, front, Outputs{target, stats, sizeof(itw_refine_target_stats), image_stats, block_sse, tier_map}, dxgi_format,
                  first_settings, refine_settings, channel_mask, *policy);
    });
}

extern "C" uint64_t itwPsnrToTotalSse(int dxgi_format, int width, int height, uint32_t channel_mask, double psnr_db)
{
    if (width < 1 || height < 1) return UINT64_MAX;
    return psnr_to_total_sse(dxgi_format, (double)width * (double)height, channel_mask, psnr_db);
}

extern "C" uint64_t itwChainPsnrToTotalSse(const rgba_surface* images, int count, int dxgi_format, uint32_t channel_mask, double psnr_db)
{
    if (!images || count < 1) return UINT64_MAX;
    double texels = 0.0;
    for (int i = 0; i < count; i++) {
        if (images[i].width < 1 || images[i].height < 1) return UINT64_MAX;
        texels += (double)images[i].width * (double)images[i].height;
    }
    return psnr_to_total_sse(dxgi_format, texels, channel_mask, psnr_db);
}
