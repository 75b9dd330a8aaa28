// etc1_core.hpp -- the arithmetic of the ETC1 encoder (kernel.ispc:3141-3691, CompressBlocksETC1_ispc), restated as the pieces a GPU mapping
// needs: what ONE lane computes for one half of a block.  Plain C++ with no HIP dependency, so that the same text runs inside the kernel
// (etc1.hip) and in a host program that walks the lanes one after the other (tools/etc1_host_check.cpp).
//
// The reference encodes a block four times -- (flip 0, diff 1), (flip 0, diff 0), (flip 1, diff 1), (flip 1, diff 0) -- and each time fits its
// two halves of 8 texels.  A half's fit has two stages:
//   stage 1  the texels sorted by R + G + B; all 165 ways to cut the sorted list into four runs (level1 <= level2 <= level3 in 0..8), each
//            scored by the best of the 8 modifier tables on the luminance alone: key = ((int)t_err << 12) + packed levels (split_key)
//   stage 2  the fastSkipTreshold smallest keys in ascending order are the candidates; each x 8 tables gets a per-channel base colour
//            (optimize_center), its quantisation (4 bits, or 5 bits clamped to -4..+3 around the first half's result) and its error on the
//            run means (eval_candidate); the first strict minimum in (candidate, table) order wins
// Stage 1 depends on the half's texels only; stage 2 on (diff, first half's result) too.
//
// Arithmetic model (the reference's ispc --opt=fast-math object code, as pinned for the other formats: x86_math.hpp):
//   x / constant          multiplies by the fp32 reciprocal of the constant (x / 255.0f, x / 8) -- except (int) / 3.0f in sort_half, which the
//                         pinned build of the reference (oracle/ref_build: an int over a float literal is the compiler's own divide there)
//                         computes as an IEEE divide.  The parity reference decides: with the reciprocal, 2 of 1 024 blocks of a noisy ramp
//                         come out different (tools/etc1_host_check.cpp)
//   1 / n, a / n          go through rcp(): RCPPS seed + one Newton step.  n is a texel count 1..8 here, so the caller passes the nine values
//                         inv[0..8] (inv[0] = 0: the reference skips empty runs)
//   a /= b                is an IEEE divide; 0 / 0 = NaN where a branch of optimize_center keeps no texel
//   min / max / clamp     are minps / maxps: the SECOND operand when unordered, so clamp(NaN, 0, hi) = 0
//   (int)f                truncates (every converted value is finite and small here)
// No multiply-add may be fused (-ffp-contract=off), no denormal flushed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ETC1_FN __host__ __device__ __forceinline__
#define ETC1_UNROLL _Pragma("unroll")           /* every array below is indexed by unrolled loop counters: registers, no scratch */
#else
#define ETC1_FN inline
#define ETC1_UNROLL
#endif

namespace itw {
namespace etc1 {

constexpr int SPLITS = 165;                     // (level1, level2, level3) with 0 <= level1 <= level2 <= level3 <= 8
constexpr int32_t KEY_NONE = 0x7fffffff;        // no key has this value: its low 12 bits would be levels (15, 15, 15)

// the intensity modifiers of the eight tables, ascending (OES_compressed_ETC1_RGB8_texture, table 3.17.2)
ETC1_FN int modifier(int table, int q)
{
    constexpr int T[8][4] = {{-8, -2, 2, 8},     {-17, -5, 5, 17},   {-29, -9, 9, 29},    {-42, -13, 13, 42},
                             {-60, -18, 18, 60}, {-80, -24, 24, 80}, {-106, -33, 33, 106}, {-183, -47, 47, 183}};
    return T[table][q];
}

// split `idx` in the reference's enumeration order, packed (level1 * 16 + level2) * 16 + level3; 0xFFF past the end
struct SplitTable { uint16_t v[176]; };
constexpr SplitTable make_split_table()
{
    SplitTable t{};
    int n = 0;
    for (int a = 0; a <= 8; a++)
        for (int b = a; b <= 8; b++)
            for (int c = b; c <= 8; c++) t.v[n++] = (uint16_t)((a * 16 + b) * 16 + c);
    for (; n < 176; n++) t.v[n] = 0xFFF;
    return t;
}

ETC1_FN float max_x86(float a, float b) { return (a > b) ? a : b; }
ETC1_FN float min_x86(float a, float b) { return (a < b) ? a : b; }
ETC1_FN float clamp_x86(float v, float lo, float hi) { return min_x86(max_x86(v, lo), hi); }
ETC1_FN float sqf(float v) { return v * v; }

// The 8 texels of a half, channel-major.  Texel kk of half `half` of a block split `flip` sits at column / row:
//   flip 0 (two 2x4 halves side by side):  col = 2 * half + (kk >> 2), row = kk & 3
//   flip 1 (two 4x2 halves, one above the other):  row = 2 * half + (kk >> 2), col = kk & 3
struct Half { float px[3][8]; };
ETC1_FN int texel_col(int flip, int half, int kk) { return flip ? (kk & 3) : 2 * half + (kk >> 2); }
ETC1_FN int texel_row(int flip, int half, int kk) { return flip ? 2 * half + (kk >> 2) : (kk & 3); }

// ---- stage 1 ------------------------------------------------------------------------------------------------------------------------------
// y[r]: a third of the r-th smallest R + G + B; rank[kk]: where texel kk stands in that order.  Ties go to the lower texel: the reference
// sorts ((int)sum << 4) + kk.
struct Sorted { float y[8]; int rank[8]; };

ETC1_FN void sort_half(const Half& h, Sorted& s)
{
    int key[8];
    ETC1_UNROLL
    for (int k = 0; k < 8; k++) {
        float value = h.px[0][k];                               // 0 + R, then + G, + B: integers, exact
        value += h.px[1][k];
        value += h.px[2][k];
        key[k] = ((int)value << 4) + k;
    }
    // rank by counting: the keys are distinct
    ETC1_UNROLL
    for (int k = 0; k < 8; k++) {
        int r = 0;
        ETC1_UNROLL
        for (int j = 0; j < 8; j++) r += (key[j] < key[k]) ? 1 : 0;
        s.rank[k] = r;
    }
    ETC1_UNROLL
    for (int r = 0; r < 8; r++) {
        int v = 0;
        ETC1_UNROLL
        for (int k = 0; k < 8; k++) v = (s.rank[k] == r) ? (key[k] >> 4) : v;
        s.y[r] = (float)v / 3.0f;                               // IEEE divide: see the model above
    }
}

// the score of one split of the sorted list: ((int)t_err << 12) + packed as a wrapping signed word
ETC1_FN int32_t split_key(const float (&y)[8], int packed, const float* inv)
{
    const int l1 = (packed >> 8) & 15, l2 = (packed >> 4) & 15, l3 = packed & 15;
    float sum[4] = {0.f, 0.f, 0.f, 0.f}, sum_sq[4] = {0.f, 0.f, 0.f, 0.f};
    int n[4] = {0, 0, 0, 0};
    ETC1_UNROLL
    for (int k = 0; k < 8; k++) {
        const int q = (k >= l1) + (k >= l2) + (k >= l3);
        const float v = y[k], vv = sqf(y[k]);
        ETC1_UNROLL
        for (int i = 0; i < 4; i++) {                            // (0 + v = v: an untouched run stays at zero like the reference's)
            const bool in = q == i;
            sum[i] = in ? sum[i] + v : sum[i];
            sum_sq[i] = in ? sum_sq[i] + vv : sum_sq[i];
            n[i] += in ? 1 : 0;
        }
    }
    float count[4], inv_count[4], mean[4];
    ETC1_UNROLL
    for (int i = 0; i < 4; i++) { count[i] = (float)n[i]; inv_count[i] = inv[n[i]]; mean[i] = sum[i] * inv_count[i]; }

    float base_err = 0.f;
    ETC1_UNROLL
    for (int i = 0; i < 4; i++) base_err += sum_sq[i] - sqf(sum[i]) * inv_count[i];

    float t_err = 256.f * 256.f * 8.f;
    ETC1_UNROLL
    for (int table = 0; table < 8; table++) {
        float center = 0.f;
        ETC1_UNROLL
        for (int i = 0; i < 4; i++) center += sum[i] - (float)modifier(table, i) * count[i];
        center *= 0.125f;                                        // /= 8: the same rounding as the IEEE divide
        float err = base_err;
        ETC1_UNROLL
        for (int i = 0; i < 4; i++) err += sqf(center + (float)modifier(table, i) - mean[i]) * count[i];
        t_err = min_x86(t_err, err);
    }
    return (int32_t)(((uint32_t)(int32_t)t_err << 12) + (uint32_t)packed);
}

// ---- stage 2 ------------------------------------------------------------------------------------------------------------------------------
// the base value of one channel for runs of mean c[q] and count n[q] under the modifiers dy[q]: the least-squares value, or that of one of
// four subsets of the runs (the others are expected to clamp), whichever reconstructs best
ETC1_FN float optimize_center(const float (&c)[4], const float (&n)[4], const float (&dy)[4])
{
    float best_center = 0.f;
    ETC1_UNROLL
    for (int q = 0; q < 4; q++) best_center += (c[q] - dy[q]) * n[q];
    best_center *= 0.125f;
    float best_err = 0.f;
    ETC1_UNROLL
    for (int q = 0; q < 4; q++) best_err += sqf(clamp_x86(best_center + dy[q], 0.f, 255.f) - c[q]) * n[q];

    ETC1_UNROLL
    for (int branch = 0; branch < 4; branch++) {
        float new_center = 0.f, sum = 0.f;
        ETC1_UNROLL
        for (int q = 0; q < 4; q++) {
            if (branch <= 1 && q <= branch) continue;
            if (branch >= 2 && q >= branch) continue;
            new_center += (c[q] - dy[q]) * n[q];
            sum += n[q];
        }
        new_center = new_center / sum;                           // IEEE; NaN when the subset is empty, which then clamps to 0 below
        float err = 0.f;
        ETC1_UNROLL
        for (int q = 0; q < 4; q++) err += sqf(clamp_x86(new_center + dy[q], 0.f, 255.f) - c[q]) * n[q];
        if (err < best_err) { best_err = err; best_center = new_center; }
    }
    return best_center;
}

// One candidate split under one table (dy: its modifiers, ascending).  `rank` as sort_half left it; `diff`: 5-bit bases (else 4-bit); `prev`: the first half's bases when this is
// the second half of a differential pair (prev[0] < 0: none).  Returns the error; qc = the quantised bases, qbits = the half's selector bits at
// their final place in the block's index word (texel at (col, row): LSB plane bit col * 4 + row, MSB plane 16 higher).
ETC1_FN float eval_candidate(const Half& h, const int (&rank)[8], int flip, int half, int packed, const float (&dy)[4], bool diff,
                             const int (&prev)[3], const float* inv, uint32_t& qbits, int (&qc)[3])
{
    const int l1 = (packed >> 8) & 15, l2 = (packed >> 4) & 15, l3 = packed & 15;
    float s[4][3] = {}, ss[4][3] = {};                           // integers below 2^24: exact in any order
    int cnt[4] = {0, 0, 0, 0};
    qbits = 0u;
    ETC1_UNROLL
    for (int kk = 0; kk < 8; kk++) {
        const int k = rank[kk];
        const int qq = (k >= l1) + (k >= l2) + (k >= l3);
        const uint32_t sel = (0x1023u >> (4 * qq)) & 3u;        // run 0..3 (ascending modifiers) -> selector 3, 2, 0, 1
        const int pos = texel_col(flip, half, kk) * 4 + texel_row(flip, half, kk);
        qbits |= ((sel & 1u) << pos) | ((sel >> 1) << (16 + pos));
        ETC1_UNROLL
        for (int q = 0; q < 4; q++) {
            const bool in = q == qq;
            cnt[q] += in ? 1 : 0;
            ETC1_UNROLL
            for (int p = 0; p < 3; p++) {
                const float v = h.px[p][kk];
                s[q][p] = in ? s[q][p] + v : s[q][p];
                ss[q][p] = in ? ss[q][p] + v * v : ss[q][p];
            }
        }
    }
    float n[4], mean[4][3], base_err = 0.f;
    ETC1_UNROLL
    for (int q = 0; q < 4; q++) {
        n[q] = (float)cnt[q];
        ETC1_UNROLL
        for (int p = 0; p < 3; p++) {
            mean[q][p] = s[q][p] * inv[cnt[q]];                  // an empty run: 0 * 0
            const float e = ss[q][p] - sqf(mean[q][p]) * n[q];
            base_err = cnt[q] > 0 ? base_err + e : base_err;
        }
    }
    float center[3];
    ETC1_UNROLL
    for (int p = 0; p < 3; p++) {
        const float c[4] = {mean[0][p], mean[1][p], mean[2][p], mean[3][p]};
        const float v = optimize_center(c, n, dy);
        const float a = v * (1.0f / 255.0f);
        if (diff) {
            int q5 = (int)clamp_x86(a * 31.0f + 0.5f, 0.f, 31.f);
            if (prev[0] >= 0) {
                if (q5 - prev[p] > 3) q5 = prev[p] + 3;
                if (q5 - prev[p] < -4) q5 = prev[p] - 4;
            }
            qc[p] = q5;
            center[p] = (float)((q5 << 3) | (q5 >> 2));
        } else {
            const int q4 = (int)clamp_x86(a * 15.0f + 0.5f, 0.f, 15.f);
            qc[p] = q4;
            center[p] = (float)((q4 << 4) | q4);
        }
    }
    float err = base_err;
    ETC1_UNROLL
    for (int q = 0; q < 4; q++)
        ETC1_UNROLL
        for (int p = 0; p < 3; p++) err += sqf(clamp_x86(center[p] + dy[q], 0.f, 255.f) - mean[q][p]) * n[q];
    return err;
}

// ---- the block word -------------------------------------------------------------------------------------------------------------------------
// qc[half][channel], table[half]; qbits: both halves' selector bits OR-ed (eval_candidate places them).  out[0] = bytes 0-3, out[1] = bytes 4-7
// of the block as little-endian words.
ETC1_FN void pack_block(const int (&qc)[2][3], const int (&table)[2], uint32_t qbits, int diff, int flip, uint32_t (&out)[2])
{
    uint32_t w = 0u;
    ETC1_UNROLL
    for (int p = 0; p < 3; p++) {
        const uint32_t byte = diff ? (((uint32_t)(qc[1][p] - qc[0][p]) & 7u) | ((uint32_t)qc[0][p] << 3))
                                   : ((uint32_t)qc[1][p] | ((uint32_t)qc[0][p] << 4));
        w |= byte << (8 * p);
    }
    w |= ((uint32_t)flip | ((uint32_t)diff << 1) | ((uint32_t)table[1] << 2) | ((uint32_t)table[0] << 5)) << 24;
    out[0] = w;
    out[1] = (qbits >> 24) | ((qbits >> 8) & 0xff00u) | ((qbits << 8) & 0xff0000u) | (qbits << 24);   // big-endian planes
}

} // namespace etc1
} // namespace itw
