// etc1.hip -- ETC1 encoder kernel for gfx950 (MI355X).
//
// Replaces kernel.ispc:3141-3691 (CompressBlocksETC1_ispc) behind itwCompressBlocksETC1 (abi.hip).  The arithmetic is etc1_core.hpp's, which
// also states the reference's algorithm; this file is the mapping.
//
// Mapping: ONE WAVE PER BLOCK, four groups of 16 lanes, one group per DISTINCT half of the block -- (flip, half) = (0,0) (0,1) (1,0) (1,1).
// The reference fits eight halves per block, but only four differ in their texels: each is fitted once with 4-bit and once with 5-bit bases.
//   stage 1  every lane of a group sorts the half's 8 texels (cheap, and it keeps the sorted list in each lane's registers), then scores 11
//            of the 165 splits (176 slots: the last 11 are padding that never wins): lane s takes splits s, s + 16, ...  The keys stay in
//            registers; nothing like the reference's int err_list[165] exists, so there is no scratch and no LDS behind it.
//   select   the reference partially sorts the list and walks its first fastSkipTreshold entries.  The keys are distinct (their low 12 bits
//            are the split itself), so "the next candidate" is the smallest key above the previous one: 11 compares per lane and a 4-step
//            xor-shuffle minimum over the group, no list and no removal state.
//   stage 2  a round evaluates two candidates x eight tables on the group's 16 lanes (lane s: candidate s >> 3 of the round, table s & 7).
//            Each lane keeps its own first strict minimum over the rounds; one ordered arg-min over the group at the end -- smallest error,
//            ties to the smallest (candidate, table) -- is the reference's first strict minimum in (candidate, table) order.
//   steps    the second half of a differential pair is clamped around the first half's result, a true dependency.  So the two fits of a half
//            run in two steps that keep all four groups busy: step 0 fits the first halves with 5-bit bases and the second halves with 4-bit
//            ones, step 1 the other way round, the second halves taking the first halves' step-0 bases from 16 lanes over.
//   block    lane 0 collects the four groups' two results each, keeps the first strict minimum in the reference's order -- flip 0 diff 1,
//            flip 0 diff 0, flip 1 diff 1, flip 1 diff 0 -- and stores the 8 bytes.
// Control flow is uniform over the wave (the round count is the threshold, a kernel argument); the lanes differ in data only.
// LDS holds nine floats: rcp(n) of the texel counts 1..8 (the only operands rcp() ever sees here) and 0 for an empty run.
//
// Loads: a lane reads its half's 8 texels as dwords; the 16 lanes of a group read the same addresses (one request per distinct dword), so a
// wave fetches its block's 64 bytes four times from L1 -- nothing next to ~10^4 VALU instructions per block.  Source base and stride must be
// 4-byte aligned, as on BC1's dword path.
#include "x86_math.hpp"
#include "kernels.hpp"
#include "etc1_core.hpp"

namespace itw {

__device__ const etc1::SplitTable ETC1_SPLITS = etc1::make_split_table();
__device__ const float ETC1_MODIFIERS[8][4] = {{-8, -2, 2, 8},     {-17, -5, 5, 17},   {-29, -9, 9, 29},    {-42, -13, 13, 42},
                                               {-60, -18, 18, 60}, {-80, -24, 24, 80}, {-106, -33, 33, 106}, {-183, -47, 47, 183}};

constexpr int ETC1_KEYS_PER_LANE = 11;          // 16 lanes x 11 = 176 >= 165
static_assert(sizeof(etc1::SplitTable) == 2 * 16 * ETC1_KEYS_PER_LANE, "one slot per (lane, key)");

// the smallest key above `prev` (`first`: any key) among the 16 lanes of a group; etc1::KEY_NONE when none is left
__device__ __forceinline__ int32_t etc1_next_key(const int32_t (&keys)[ETC1_KEYS_PER_LANE], int32_t prev, bool first)
{
    int32_t m = etc1::KEY_NONE;
#pragma unroll
    for (int j = 0; j < ETC1_KEYS_PER_LANE; j++) {
        const int32_t k = keys[j];
        m = ((first || k > prev) && k < m) ? k : m;
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) m = min(m, __shfl_xor(m, off));      // partners stay inside the aligned group of 16
    return m;
}

// A half's fit: error, (candidate * 8 + table) of the winner, its selector bits and its bases (5 bits each at 0, 5, 10).  Kept as four words and
// updated word by word with one condition: a select between two whole structs goes through their addresses, that is through scratch.
struct Etc1Fit { float err; int32_t order; uint32_t qbits; int32_t qc; };

__device__ __forceinline__ void etc1_take(Etc1Fit& f, bool c, float err, int32_t order, uint32_t qbits, int32_t qc)      // if (c) f = {...}
{
    f.err = c ? err : f.err; f.order = c ? order : f.order; f.qbits = c ? qbits : f.qbits; f.qc = c ? qc : f.qc;
}
// smaller error, ties to the smaller (candidate, table)
__device__ __forceinline__ void etc1_merge(Etc1Fit& f, float err, int32_t order, uint32_t qbits, int32_t qc)
{
    const bool c = (err < f.err) | ((err == f.err) & (order < f.order));
    etc1_take(f, c, err, order, qbits, qc);
}

// `threshold` in 1 .. 165.  One wave per block: grid = ceil(nblocks / 4) workgroups of 4 waves.
__global__ void __launch_bounds__(256)
etc1_kernel(const uint8_t* __restrict__ src, int64_t stride, int32_t blocks_x, int32_t nblocks, uint8_t* __restrict__ dst, int32_t threshold)
{
    __shared__ float s_inv[16];
    if (threadIdx.x < 9) s_inv[threadIdx.x] = threadIdx.x ? ispc_rcp((float)threadIdx.x, global_seed_tables()) : 0.f;
    __syncthreads();

    const int32_t b = (int32_t)blockIdx.x * 4 + (int32_t)(threadIdx.x >> 6);     // wave-uniform
    if (b >= nblocks) return;
    const int lane = threadIdx.x & 63, sub = lane & 15;
    const int flip = lane >> 5, half = (lane >> 4) & 1, table = sub & 7, slot = sub >> 3;
    float dy[4];
#pragma unroll
    for (int q = 0; q < 4; q++) dy[q] = ETC1_MODIFIERS[table][q];

    const int32_t yy = b / blocks_x, xx = b - yy * blocks_x;
    etc1::Half h;
#pragma unroll
    for (int kk = 0; kk < 8; kk++) {
        const int row = etc1::texel_row(flip, half, kk), col = etc1::texel_col(flip, half, kk);
        const uint32_t t = *reinterpret_cast<const uint32_t*>(src + ((int64_t)yy * 4 + row) * stride + ((int64_t)xx * 4 + col) * 4);
        h.px[0][kk] = (float)(t & 255u); h.px[1][kk] = (float)((t >> 8) & 255u); h.px[2][kk] = (float)((t >> 16) & 255u);
    }

    // stage 1: this lane's 11 of the half's 165 keys
    etc1::Sorted s;
    etc1::sort_half(h, s);
    int32_t keys[ETC1_KEYS_PER_LANE];
#pragma unroll
    for (int j = 0; j < ETC1_KEYS_PER_LANE; j++) {
        const int packed = ETC1_SPLITS.v[sub + 16 * j];
        const int32_t k = etc1::split_key(s.y, packed, s_inv);
        keys[j] = packed == 0xFFF ? etc1::KEY_NONE : k;
    }

    // stage 2, twice: (half 0, diff 1) and (half 1, diff 0), then (half 0, diff 0) and (half 1, diff 1 around half 0's step-0 bases)
    Etc1Fit fit[2] = {};                             // [diff]
    int32_t first_half_qc = 0;
#pragma unroll
    for (int step = 0; step < 2; step++) {
        const bool diff = (half == 0) == (step == 0);
        int prev[3] = {-1, -1, -1};
        if (step == 1) {
            const int32_t other = __shfl_xor(first_half_qc, 16);
            if (half == 1) { prev[0] = other & 31; prev[1] = (other >> 5) & 31; prev[2] = (other >> 10) & 31; }
        }
        Etc1Fit best{255.f * 255.f * 3.f * 8.f, 0x7fffffff, 0u, 0};
        int32_t last = 0;
        for (int i = 0; i < threshold; i += 2) {
            const int32_t k0 = etc1_next_key(keys, last, i == 0), k1 = etc1_next_key(keys, k0, false);
            last = k1;
            const int cand = i + slot;
            uint32_t qbits;
            int qc[3];
            const float err = etc1::eval_candidate(h, s.rank, flip, half, (slot ? k1 : k0) & 0xFFF, dy, diff, prev, s_inv, qbits, qc);
            etc1_take(best, (cand < threshold) & (err < best.err), err, cand * 8 + table, qbits, qc[0] | (qc[1] << 5) | (qc[2] << 10));
        }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1)
            etc1_merge(best, __shfl_xor(best.err, off), __shfl_xor(best.order, off), (uint32_t)__shfl_xor((int)best.qbits, off), __shfl_xor(best.qc, off));
        if (step == 0) first_half_qc = best.qc;      // (read by the second halves only, from the first halves' lanes)
        etc1_take(fit[0], !diff, best.err, best.order, best.qbits, best.qc);
        etc1_take(fit[1], diff, best.err, best.order, best.qbits, best.qc);
    }

    // the block: the four (flip, diff) encodings in the reference's order, first strict minimum
    float best_err = __builtin_inff();
    uint32_t out[2] = {0u, 0u};
#pragma unroll
    for (int f = 0; f < 2; f++)
#pragma unroll
        for (int d = 1; d >= 0; d--) {
            const Etc1Fit& m = fit[d];
            const Etc1Fit a{__shfl(m.err, f * 32), __shfl(m.order, f * 32), (uint32_t)__shfl((int)m.qbits, f * 32), __shfl(m.qc, f * 32)};
            const Etc1Fit c{__shfl(m.err, f * 32 + 16), __shfl(m.order, f * 32 + 16), (uint32_t)__shfl((int)m.qbits, f * 32 + 16), __shfl(m.qc, f * 32 + 16)};
            float err = a.err;                       // 0 + a
            err += c.err;
            const int qc[2][3] = {{a.qc & 31, (a.qc >> 5) & 31, (a.qc >> 10) & 31}, {c.qc & 31, (c.qc >> 5) & 31, (c.qc >> 10) & 31}};
            const int tables[2] = {a.order & 7, c.order & 7};
            uint32_t w[2];
            etc1::pack_block(qc, tables, a.qbits | c.qbits, d, f, w);
            const bool better = err < best_err;
            best_err = better ? err : best_err;
            out[0] = better ? w[0] : out[0];
            out[1] = better ? w[1] : out[1];
        }
    if (lane == 0) {
        uint32_t* o = reinterpret_cast<uint32_t*>(dst + (int64_t)b * 8);
        o[0] = out[0]; o[1] = out[1];
    }
}

// `threshold` >= 1 (abi.hip refuses the rest); above 165 every split is already a candidate
void launch_etc1(const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, int threshold, hipStream_t st)
{
    const int bx = width / 4, by = height / 4;
    const int64_t n = (int64_t)bx * by;
    if (n <= 0) return;
    const int t = threshold > etc1::SPLITS ? etc1::SPLITS : threshold;
    hipLaunchKernelGGL(etc1_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, src, stride, bx, (int32_t)n, dst, (int32_t)t);
}

} // namespace itw
