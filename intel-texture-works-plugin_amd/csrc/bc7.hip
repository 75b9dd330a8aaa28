// bc7.hip -- BC7 encoder kernels for gfx950 (MI355X).
//
// Replaces kernel.ispc:616-2037 (CompressBlocksBC7_ispc) behind CompressBlocksBC7
// (ispc_texcomp.cpp:427-430).  Same search as the reference -- PCA line fits per
// subset, p-bit aware endpoint quantisation, two-candidate index selection,
// least-squares refinement of each mode's winner, modes 0-7 -- organised for a
// SIMT machine instead of an SPMD gang:
//
//   * one 4x4 block per lane, read from HBM with 4 coalesced dwordx4 loads per lane,
//     16 B written per lane.  The block lives in 16 VGPRs as loaded plus 16 VGPRs of
//     planar bytes (bc7_exact.hpp);
//   * everything the reference computes in fp32 that cannot round (texels and decoded
//     endpoints are integers <= 255) runs on the packed integer units: subset moment
//     sums are masked v_dot4_u32_u8 chains, index selection projects with v_dot2 and an
//     exactly rounded quotient and compares the two candidate indices through per-segment
//     palettes in LDS (one v_dot4 per candidate), least-squares sums are dot4 chains
//     (proofs in bc7_exact.hpp).  What can round (PCA, endpoint quantisation, the 2x2
//     solve) is fp32 with the pinned x86 arithmetic;
//   * the SCANS of the shapes (110-128 VGPRs, 4 waves per SIMD) and the REFINEMENT of each mode's winner (per-lane shapes,
//     2 waves per SIMD) have different register budgets and therefore live in different kernels; how many launches a call
//     takes depends on its size (bottom of this file): whole surfaces run FUSED (bc7_scan_all: the scans of families {0,2}
//     and {1,3} in one launch, XCD-aware so the second family reads its texels from L2; bc7_finish_all: every mode's
//     refinement + modes 4/5/6 in one launch), calls too small to fill the chip run WIDE (each scan split over several
//     waves, winners joined by an ordered argmin, single-subset modes on a second stream).  Families run in the
//     reference's order and only communicate through "best error so far" (kernel.ispc:1358, 1638, 1684) and the search
//     winners; the per-family search / finish kernel pairs of round 1 remain for ranked lists longer than 16 shapes.
//     The slow profiles (every shape scanned) run the BOUNDED order instead (round 4: modes 1/3/7 last, only for the blocks an
//     exact lower bound cannot exclude, compacted into lists) as two interleaved bands on two streams, and for the RGB
//     profile a pilot kernel picks that order or the reference's per call, on the device (round 5; launch_rgb_bounded);
//     under the RGB profile the list scan of that order fits only the (block, shape) pairs the bound leaves (PAIRS, above bc7_pair_scan):
//     bc7_bounded_setup (counters, where the pairs go) -> bc7_scan_all {0,2} per band -> bc7_pilot_estimate -> bc7_finish_all<3> (modes 0,2,4,5,6,
//     the 64 bounds once, the list, the compact texels and the pairs bucketed by shape) -> bc7_pair_scan -> bc7_finish_all<8> -> the full list
//     scan and bc7_finish_all<4> for the few blocks it defers;
//   * the scans produce a candidate's ERROR and nothing else: the level a texel takes
//     and the packed indices matter for a mode's winner alone, so the winner record is
//     {error, shape} and the finish kernel recomputes endpoints and indices of the
//     winner (same inputs, same bits) before refining it;
//   * shapes are visited in a wave-uniform order wherever the candidate list is the
//     whole table (modes 0/2 always; modes 1/3/7 when their fastSkipTreshold is >= 64,
//     the `slow` profiles): subset masks are scalars, a texel costs work only in the
//     subset it belongs to (scalar branches), and the loop over subsets is rolled so
//     every code path exists once.  The reference scans its PCA-ranked list with a
//     strict `<`, i.e. among equal errors the lowest rank key wins; here the rank key
//     (part + 64*bound) is only evaluated when two shapes actually tie;
//   * modes 0/2: a subset's mode 2 result depends on its texel mask alone and 192
//     subsets use 140 masks, so the scan follows a generated schedule that clusters
//     equal masks and reloads results from a four-entry register cache;
//   * shorter ranked lists (fast profiles) keep the per-lane order: the i-th entry of
//     the reference's selection sort (kernel.ispc:1365-1384) is the i-th smallest key --
//     the 16 smallest are kept sorted in registers while the keys are produced (every
//     preset; longer custom lists scan 64 keys in LDS), no dynamic register indexing;
//   * fits that do not depend on the mode are shared: shapes 64..79 serve modes 0 and
//     2, every two-subset shape serves modes 1 and 3 (kernel.ispc:1286-1291), the last
//     subset's moments are the block's minus the others' (exact), one rotation's fit
//     serves its three mode 4/5 candidates;
//   * the RCPPS/RSQRTPS seed tables are staged in LDS once per workgroup.
//
// VALU issue bound; nothing GEMM shaped, so no MFMA.  Bit-exactness with
// the oracle forbids FMA contraction and any re-association of sums that can round.
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include "bc7_exact.hpp"
#include "kernels.hpp"
#include "host_rt.hpp"
#ifdef ITW_TEST_HOOKS
#include "../../include/itw_test_hooks.h"
#endif

namespace itw {

#define BCN_TABLE_QUAL __device__ const
#include "bc7_f02_schedule.h"
#undef BCN_TABLE_QUAL

// per-lane shapes (refinement, ranked lists <= 16) go through per-subset palettes in LDS (bc7_exact.hpp)
constexpr int LANE_PAL_LEVELS = 24;       // 3 subsets x 8 levels: the most one mode's refinement decodes (48 KiB per workgroup)
constexpr int TPB = 256;                  // four waves share one staged seed table
constexpr float INV255 = 1.0f / 255.0f;   // x/255f under fast-math = x*(1.f/255.f)
constexpr int32_t ERR_MAX = 0x7fffffff;
enum Family { F_MODES02 = 0, F_MODES13 = 1, F_MODE7 = 2, F_MODES456 = 3 };

struct ModeTraits { int pairs, bits, ch; };
__device__ __forceinline__ constexpr ModeTraits traits(int mode)
{
    return mode == 0 ? ModeTraits{3, 3, 3} : mode == 1 ? ModeTraits{2, 3, 3} : mode == 2 ? ModeTraits{3, 2, 3}
         : mode == 3 ? ModeTraits{2, 2, 3} : ModeTraits{2, 2, 4} /* 7 */;
}

__device__ __forceinline__ int32_t expand_to_byte(int32_t v, int bits)        // kernel.ispc:976-981
{
    const int32_t vv = v << (8 - bits);
    return vv + (int32_t)((uint32_t)vv >> bits);
}

// float -> int of the reference (cvttps2dq).  SAFE: the caller guarantees a finite value inside the int range
// (search-time endpoints are clamped to [0,255] by the fit), so the plain conversion gives the same result.
template <bool SAFE>
__device__ __forceinline__ int32_t f2i(float f) { return SAFE ? (int32_t)f : f2i_x86(f); }

// ---- endpoint quantisers --------------------------------------------------------------------------
// in : e[i][p]  fitted endpoint i, channel p (fp32)
// out: q[i][p]  code as stored in the block (incl. p-bit in bit 0 where the mode has one)
//      d[i][p]  what a decoder reconstructs from it (the reference overwrites e with this; kernel.ispc:1100-1128)

// modes 0,3,6,7: one p-bit per endpoint, chosen by squared error over `err_ch` channels.  [kernel.ispc:983-1022]
// SAFE (fitted endpoints, clamped to [0,255]): u = (e/255*L2 - b)/2 + 0.5 is in [0, 2^BITS + 1), so the code
// 2*floor(u) + b stays an integer-valued float end to end (floor, *2, +b are exact) and only the chosen hypothesis is
// converted; of the reference's clamp [b, L2-1+b] only the upper bound of b = 0 can fire (u >= 2^BITS needs
// e/255*L2 >= L2, i.e. e = 255; for b = 1, u < 2^BITS always).  Modes 3, 6, 7 compare the code itself (kernel.ispc:
// 1003-1017: mode 7 compares raw 6-bit codes against 8-bit targets, a reference quirk), mode 0 its 5-bit expansion.
// For b = 1 the reference's u = (t - 1)*0.5 + 0.5 equals t*0.5 exactly when t >= 0.5 (t - 1 is then exact, the rest
// is scaling and an exactly representable sum); for t < 0.5 both floors are 0.  SAFE paths use floor(t*0.5) directly.
// Round 4: mode 0 (4 bits + p-bit, compared through its 5-bit expansion) and mode 1 (shared p-bit, 7-bit expansion) take the same
// float-domain route in the scans: a code c is an integer-valued float, and expand_to_byte(c, BITS) = c * 2^(8-BITS) + (c >> (2*BITS-8))
// is c * 8 + floor(c / 4) for 5 bits and c * 2 + [c >= 64] for 7 bits -- exact in fp32 (small integers, power-of-two scalings) -- so
// the hypotheses' decoded values are formed without a float -> int -> float round trip per value (the integer route costs a
// conversion each way plus a shift, a bit-field extract and an add, all 4-cycle forms; tests/test_exact_forms.py walks every code).
template <int MODE, bool SAFE>
__device__ __forceinline__ void quant_pbit(int32_t (&q)[2][4], int32_t (&d)[2][4], const float (&e)[2][4], int err_ch)
{
    constexpr int BITS = (MODE == 0) ? 4 : (MODE == 7) ? 5 : 7;
    constexpr int L2 = (1 << BITS) * 2 - 1;
    #pragma unroll
    for (int i = 0; i < 2; i++) {
        if (SAFE) {
            float cb[2][4], db[2][4];          // code incl. p-bit / what the error is measured against, per hypothesis
            #pragma unroll
            for (int p = 0; p < 4; p++) {
                const float t = e[i][p] * INV255 * (float)L2;
                const float v0 = __builtin_floorf(t * 0.5f + 0.5f) * 2.0f;
                cb[0][p] = __builtin_fminf(v0, (float)(L2 - 1));                   // v0 is an ordinary number here (SAFE)
                cb[1][p] = __builtin_floorf(t * 0.5f) * 2.0f + 1.0f;       // (t-1)/2 + 1/2 = t/2 exactly for t >= 0.5, floor 0 below
                #pragma unroll
                for (int b = 0; b < 2; b++)
                    db[b][p] = (MODE == 0) ? cb[b][p] * 8.0f + __builtin_floorf(cb[b][p] * 0.25f) : cb[b][p];   // mode 0: 5-bit code -> byte
            }
            float err0 = 0.f, err1 = 0.f;
            #pragma unroll
            for (int p = 0; p < 4; p++)
                if (p < err_ch) { err0 += sq(e[i][p] - db[0][p]); err1 += sq(e[i][p] - db[1][p]); }
            const bool first = err0 < err1;
            #pragma unroll
            for (int p = 0; p < 4; p++) {
                q[i][p] = (int32_t)(first ? cb[0][p] : cb[1][p]);
                d[i][p] = (MODE == 7) ? expand_to_byte(q[i][p], 6) : (MODE == 0) ? (int32_t)(first ? db[0][p] : db[1][p]) : q[i][p];
            }
            continue;
        }
        int32_t qb[2][4];
        float db[2][4];
        #pragma unroll
        for (int b = 0; b < 2; b++)
            #pragma unroll
            for (int p = 0; p < 4; p++) {
                const float t = e[i][p] * INV255 * (float)L2;
                const float u = (t - (float)b) * 0.5f + 0.5f;
                const uint32_t v = (uint32_t)f2i<SAFE>(u) * 2u + (uint32_t)b;
                qb[b][p] = iclamp((int32_t)v, b, L2 - 1 + b);
                // mode 0 compares in 8-bit space; modes 3/6 codes are 8-bit; mode 7 compares raw 6-bit codes
                // against 8-bit targets (reference quirk, kernel.ispc:1003-1017)
                db[b][p] = (float)((MODE == 0) ? expand_to_byte(qb[b][p], 5) : qb[b][p]);
            }
        float err0 = 0.f, err1 = 0.f;
        #pragma unroll
        for (int p = 0; p < 4; p++)
            if (p < err_ch) { err0 += sq(e[i][p] - db[0][p]); err1 += sq(e[i][p] - db[1][p]); }
        const bool first = err0 < err1;
        #pragma unroll
        for (int p = 0; p < 4; p++) {
            q[i][p] = first ? qb[0][p] : qb[1][p];
            d[i][p] = (MODE == 0) ? expand_to_byte(q[i][p], 5) : (MODE == 7) ? expand_to_byte(q[i][p], 6) : q[i][p];
        }
    }
}

// mode 1: one p-bit shared by both endpoints of a subset, RGB error.            [kernel.ispc:1024-1052]
template <bool SAFE>
__device__ __forceinline__ void quant_shared_pbit(int32_t (&q)[2][4], int32_t (&d)[2][4], const float (&e)[2][4])
{
    if (SAFE) {
        // float domain (see quant_pbit): code c in [0, 127], decoded byte c * 2 + (c >> 6) = c + c + [c >= 64]
        float cb[2][2][4], db[2][2][4];
        #pragma unroll
        for (int i = 0; i < 2; i++)
            #pragma unroll
            for (int p = 0; p < 4; p++) {
                const float t = e[i][p] * INV255 * 127.0f;
                const float v0 = __builtin_floorf(t * 0.5f + 0.5f) * 2.0f;
                cb[0][i][p] = __builtin_fminf(v0, 126.0f);
                cb[1][i][p] = __builtin_floorf(t * 0.5f) * 2.0f + 1.0f;
                #pragma unroll
                for (int b = 0; b < 2; b++)
                    db[b][i][p] = cb[b][i][p] * 2.0f + __builtin_floorf(cb[b][i][p] * 0.015625f);
            }
        float err0 = 0.f, err1 = 0.f;
        #pragma unroll
        for (int i = 0; i < 2; i++)
            #pragma unroll
            for (int p = 0; p < 3; p++) { err0 += sq(e[i][p] - db[0][i][p]); err1 += sq(e[i][p] - db[1][i][p]); }
        const bool first = err0 < err1;
        #pragma unroll
        for (int i = 0; i < 2; i++)
            #pragma unroll
            for (int p = 0; p < 4; p++) {
                q[i][p] = (int32_t)(first ? cb[0][i][p] : cb[1][i][p]);
                d[i][p] = (int32_t)(first ? db[0][i][p] : db[1][i][p]);
            }
        return;
    }
    int32_t qb[2][2][4];
    float db[2][2][4];
    #pragma unroll
    for (int b = 0; b < 2; b++)
        #pragma unroll
        for (int i = 0; i < 2; i++)
            #pragma unroll
            for (int p = 0; p < 4; p++) {
                const float t = e[i][p] * INV255 * 127.0f;
                const float u = (t - (float)b) * 0.5f + 0.5f;
                const uint32_t v = (uint32_t)f2i<SAFE>(u) * 2u + (uint32_t)b;
                qb[b][i][p] = iclamp((int32_t)v, b, 126 + b);
                db[b][i][p] = (float)expand_to_byte(qb[b][i][p], 7);
            }
    float err0 = 0.f, err1 = 0.f;
    #pragma unroll
    for (int i = 0; i < 2; i++)
        #pragma unroll
        for (int p = 0; p < 3; p++) { err0 += sq(e[i][p] - db[0][i][p]); err1 += sq(e[i][p] - db[1][i][p]); }
    const bool first = err0 < err1;
    #pragma unroll
    for (int i = 0; i < 2; i++)
        #pragma unroll
        for (int p = 0; p < 4; p++) {
            q[i][p] = first ? qb[0][i][p] : qb[1][i][p];
            d[i][p] = expand_to_byte(q[i][p], 7);
        }
}

// modes 2,4 (5 bits) and 5 (7 bits): plain rounding.                            [kernel.ispc:1054-1065]
template <int BITS, bool SAFE>
__device__ __forceinline__ void quant_plain(int32_t (&q)[2][4], int32_t (&d)[2][4], const float (&e)[2][4])
{
    constexpr int L = 1 << BITS;
    #pragma unroll
    for (int i = 0; i < 2; i++)
        #pragma unroll
        for (int p = 0; p < 4; p++) {
            const int32_t v = f2i<SAFE>(e[i][p] * INV255 * (float)(L - 1) + 0.5f);
            q[i][p] = SAFE ? v : iclamp(v, 0, L - 1);          // e in [0,255]: e/255*(L-1) + 0.5 < L, never negative
            d[i][p] = expand_to_byte(q[i][p], BITS);
        }
}

template <int MODE, bool SAFE>
__device__ __forceinline__ void quant_mode(int32_t (&q)[2][4], int32_t (&d)[2][4], const float (&e)[2][4], int err_ch)
{
    if (MODE == 0 || MODE == 3 || MODE == 6 || MODE == 7) quant_pbit<MODE, SAFE>(q, d, e, err_ch);
    else if (MODE == 1) quant_shared_pbit<SAFE>(q, d, e);
    else if (MODE == 2 || MODE == 4) quant_plain<5, SAFE>(q, d, e);
    else quant_plain<7, SAFE>(q, d, e);
}

// ---- per-lane state ---------------------------------------------------------------------------
// All BC7 block errors are exact integers below 2^24 in the reference's float arithmetic (sums of per-texel
// `(int)err`, plus the integer opaque_err), so they are carried as int32 here; +inf is ERR_MAX.
struct Lane {
    Tex tx;
    int32_t best_err;
    int32_t opaque_err;
    uint32_t best[4];
    bool improved;
    SeedTables T;
    int32_t* keys;            // LDS column (ranked-list path only): keys[i * TPB]
    uint2* pal;               // LDS column of palettes (table-order scans): 12 levels, pal[level * TPB]; levels 12, 13: search_02<true>'s mode 0 cache
};

struct Win {                  // winner of one multi-subset mode during the search (its indices are recomputed by the finish kernel)
    int32_t err;
    int32_t shape;            // table index 0..63 (two subsets) / 64..127 (three)
    int32_t key;              // rank key of `shape`; < 0 = not evaluated yet (table-order scans)
};

__device__ __forceinline__ void reset(Win& w, int shape0)
{
    w.err = ERR_MAX;
    w.shape = shape0;
    w.key = -1;
}

__device__ __forceinline__ void store_bits(uint32_t (&out)[4], const BlockBits& bb)
{
    out[0] = (uint32_t)bb.lo; out[1] = (uint32_t)(bb.lo >> 32); out[2] = (uint32_t)bb.hi; out[3] = (uint32_t)(bb.hi >> 32);
}

// ---- bitstream --------------------------------------------------------------------------------
// modes 0,1,2,3,7                                                        [kernel.ispc:1708-1733, 1767-1877]
template <int MODE>
__device__ __forceinline__ void emit_multi(uint32_t (&out)[4], int32_t (&cq)[3][2][4], const uint32_t (&cqb)[2], int shape)
{
    constexpr ModeTraits M = traits(MODE);
    constexpr int LEVELS = 1 << M.bits;
    const Shape sh = load_shape(shape);
    const int a1 = (int)(sh.anchors >> 4), a2 = (int)(sh.anchors & 15u);

    // an anchor index must have its top bit clear: swap the subset's endpoints and mirror its indices
    uint32_t flips = 0;
    #pragma unroll
    for (int j = 0; j < M.pairs; j++) {
        const int k0 = (j == 0) ? 0 : ((j == 1) ? a1 : a2);
        const uint32_t word = (k0 < 8) ? cqb[0] : cqb[1];
        const int32_t q = (int32_t)((word >> (4 * (k0 & 7))) & 15u);
        if (q >= LEVELS / 2) {
            #pragma unroll
            for (int p = 0; p < 4; p++) { const int32_t t = cq[j][0][p]; cq[j][0][p] = cq[j][1][p]; cq[j][1][p] = t; }
            flips |= subset_mask(sh, j);
        }
    }

    BlockBits bb;
    int pos = 0;
    bb.put(pos, MODE + 1, 1u << MODE); pos += MODE + 1;
    if (MODE == 0) { bb.put(pos, 4, (uint32_t)shape & 15u); pos += 4; }
    else           { bb.put(pos, 6, (uint32_t)shape & 63u); pos += 6; }

    constexpr int EPB = (MODE == 0) ? 4 : (MODE == 1) ? 6 : (MODE == 2) ? 5 : (MODE == 3) ? 7 : 5;
    constexpr bool HAS_P = (MODE != 2);
    #pragma unroll
    for (int p = 0; p < M.ch; p++)
        #pragma unroll
        for (int j = 0; j < M.pairs; j++)
            #pragma unroll
            for (int i = 0; i < 2; i++) {
                bb.put(pos, EPB, (uint32_t)(HAS_P ? (cq[j][i][p] >> 1) : cq[j][i][p]));
                pos += EPB;
            }
    if (MODE == 1) {
        #pragma unroll
        for (int j = 0; j < 2; j++) { bb.put(pos, 1, (uint32_t)cq[j][0][0] & 1u); pos += 1; }
    } else if (HAS_P) {
        #pragma unroll
        for (int j = 0; j < M.pairs; j++)
            #pragma unroll
            for (int i = 0; i < 2; i++) { bb.put(pos, 1, (uint32_t)cq[j][i][0] & 1u); pos += 1; }
    }

    const int start = pos;                                   // = 128 + (pairs-1) - (16*bits - 1)
    #pragma unroll
    for (int k = 0; k < 16; k++) {
        uint32_t q = ((k < 8 ? cqb[0] >> (4 * k) : cqb[1] >> (4 * (k - 8))) & 15u);
        if ((flips >> k) & 1u) q = (uint32_t)(LEVELS - 1) - q;
        const int n = (k == 0) ? M.bits - 1 : M.bits;
        bb.put(pos, n, q); pos += n;
    }
    // delete the (zero) top bit of the other anchors, highest position first
    const int msb1 = start + M.bits * a1 + M.bits - 2;
    if (M.pairs == 3) {
        const int msb2 = start + M.bits * a2 + M.bits - 2;
        bb.drop_bit(max(msb1, msb2));
        bb.drop_bit(min(msb1, msb2));
    } else {
        bb.drop_bit(msb1);
    }
    store_bits(out, bb);
}

// single-subset anchor rule for modes 4,5,6                                       [kernel.ispc:1694-1706]
template <int BITS, int NCH>
__device__ __forceinline__ void fix_anchor(int32_t (&e0)[NCH], int32_t (&e1)[NCH], uint32_t (&qb)[2])
{
    constexpr uint32_t L = 1u << BITS;
    if ((qb[0] & 15u) >= L / 2) {
        #pragma unroll
        for (int p = 0; p < NCH; p++) { const int32_t t = e0[p]; e0[p] = e1[p]; e1[p] = t; }
        qb[0] = 0x11111111u * (L - 1) - qb[0];
        qb[1] = 0x11111111u * (L - 1) - qb[1];
    }
}

template <int BITS>
__device__ __forceinline__ void put_indices(BlockBits& bb, int& pos, const uint32_t (&qb)[2])
{
    #pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t q = ((k < 8 ? qb[0] >> (4 * k) : qb[1] >> (4 * (k - 8))) & 15u);
        const int n = (k == 0) ? BITS - 1 : BITS;
        bb.put(pos, n, q); pos += n;
    }
}

struct Dual {                 // a mode 4/5 candidate: vector part + scalar part
    int32_t q[2][4];          // colour endpoints (slot 3 unused)
    uint32_t qb[2];
    int32_t aq[2];            // scalar channel endpoints
    uint32_t aqb[2];
    int32_t rotation, swap;
};

// modes 4 and 5                                                                   [kernel.ispc:1879-1939]
template <int MODE>
__device__ __forceinline__ void emit_dual(uint32_t (&out)[4], const Dual& d)
{
    constexpr int ABITS = (MODE == 4) ? 3 : 2, EPB = (MODE == 4) ? 5 : 7, AEPB = (MODE == 4) ? 6 : 8;
    int32_t c0[4], c1[4], a0[1], a1[1];
    uint32_t vb[2] = {d.qb[0], d.qb[1]}, sb[2] = {d.aqb[0], d.aqb[1]};
    #pragma unroll
    for (int p = 0; p < 4; p++) { c0[p] = d.q[0][p]; c1[p] = d.q[1][p]; }
    a0[0] = d.aq[0]; a1[0] = d.aq[1];
    if (!d.swap) {
        fix_anchor<2, 4>(c0, c1, vb);
        fix_anchor<ABITS, 1>(a0, a1, sb);
    } else {
        // index sets trade places: the 2-bit set (now the scalar's) is stored first
        uint32_t t0 = vb[0], t1 = vb[1]; vb[0] = sb[0]; vb[1] = sb[1]; sb[0] = t0; sb[1] = t1;
        fix_anchor<2, 1>(a0, a1, vb);
        fix_anchor<ABITS, 4>(c0, c1, sb);
    }
    BlockBits bb;
    int pos = 0;
    bb.put(pos, MODE + 1, 1u << MODE); pos += MODE + 1;
    bb.put(pos, 2, (uint32_t)(d.rotation + 1) & 3u); pos += 2;
    if (MODE == 4) { bb.put(pos, 1, (uint32_t)d.swap); pos += 1; }
    #pragma unroll
    for (int p = 0; p < 3; p++) {
        bb.put(pos, EPB, (uint32_t)c0[p]); pos += EPB;
        bb.put(pos, EPB, (uint32_t)c1[p]); pos += EPB;
    }
    bb.put(pos, AEPB, (uint32_t)a0[0]); pos += AEPB;
    bb.put(pos, AEPB, (uint32_t)a1[0]); pos += AEPB;
    put_indices<2>(bb, pos, vb);
    put_indices<ABITS>(bb, pos, sb);
    store_bits(out, bb);
}

// mode 6                                                                          [kernel.ispc:1941-1964]
__device__ __forceinline__ void emit_mode6(uint32_t (&out)[4], int32_t (&q)[2][4], uint32_t (&qb)[2])
{
    fix_anchor<4, 4>(q[0], q[1], qb);
    BlockBits bb;
    int pos = 0;
    bb.put(pos, 7, 64u); pos += 7;
    #pragma unroll
    for (int p = 0; p < 4; p++) {
        bb.put(pos, 7, (uint32_t)(q[0][p] >> 1)); pos += 7;
        bb.put(pos, 7, (uint32_t)(q[1][p] >> 1)); pos += 7;
    }
    bb.put(pos, 1, (uint32_t)q[0][0] & 1u); pos += 1;
    bb.put(pos, 1, (uint32_t)q[1][0] & 1u); pos += 1;
    put_indices<4>(bb, pos, qb);
    store_bits(out, bb);
}

// ---- multi-subset modes ---------------------------------------------------------------------

// Rank key of a two-subset shape: shape + 64 * (int)(sqrt(residual bound) * 256).   [kernel.ispc:952-971, 1404-1409]
// `shape` may differ per lane (table loads are then per lane).
template <int RANK_CH>
__device__ __forceinline__ int32_t rank_key(int shape, const Tex& tx, const Stats<RANK_CH>& full, const SeedTables& T)
{
    const SubsetMask sm = subset_of(shape, 0);
    IStats<RANK_CH> s0;
    stats_int<RANK_CH>(s0, tx.pl, sm);
    Stats<RANK_CH> f0;
    stats_float<RANK_CH>(f0, s0);
    return (int32_t)((uint32_t)shape + (uint32_t)split_bound_from<RANK_CH, true>(f0, full, T, rcp_of_count(sm.n), rcp_of_count(16 - sm.n)) * 64u);
}

// Least-squares refinement of a mode's winner, then the mode competes for the block.  [kernel.ispc:1329-1362]
// The winner's shape differs per lane: masks come from per-lane table loads, segments are chosen per texel.
template <int MODE>
__device__ __forceinline__ void refine_and_commit(Lane& ln, Win& w, int iterations, int settings_channels)
{
    constexpr ModeTraits M = traits(MODE);
    const Shape sh = load_shape(w.shape);
    SubsetMask sm[3];
    #pragma unroll
    for (int j = 0; j < M.pairs; j++) sm[j] = subset_of(w.shape, j);
    // endpoint codes and indices of the search-time winner: the scan kept only its error, so refit + quantise its
    // shape again (same inputs, same bits) and select once; the error found equals w.err
    int32_t cq[3][2][4];
    uint32_t wqb[2];
    #pragma unroll
    for (int j = 0; j < 3; j++) for (int i = 0; i < 2; i++) for (int p = 0; p < 4; p++) cq[j][i][p] = 0;
    constexpr int LEVELS = 1 << M.bits;
    const int32_t tt = block_norm2<M.ch>(ln.tx.pl);
    {
        PalSegment sg0[3];
        #pragma unroll 1
        for (int j = 0; j < M.pairs; j++) {
            const SubsetMask s = subset_of(w.shape, j);       // (selecting among sm[0..2] here made the compiler index them in scratch)
            IStats<M.ch> st;
            stats_int<M.ch>(st, ln.tx.pl, s);
            float ep[2][4];
            ep[0][3] = 0.f; ep[1][3] = 0.f;
            fit_line<M.ch>(ep, ln.tx, s.bits, st, ispc_rcp((float)s.n, ln.T), ln.T);
            int32_t q[2][4], d[2][4];
            quant_mode<MODE, true>(q, d, ep, M.ch);
            const PalSegment sgj = build_palette<M.bits, M.ch, TPB>(ln.pal + j * (LEVELS * TPB), d);
            #pragma unroll
            for (int i = 0; i < 2; i++) for (int p = 0; p < 4; p++) {
                if (j == 0) cq[0][i][p] = q[i][p]; else if (j == 1) cq[1][i][p] = q[i][p]; else cq[2][i][p] = q[i][p];
            }
            if (j == 0) sg0[0] = sgj; else if (j == 1) sg0[1] = sgj; else sg0[2] = sgj;
        }
        if (M.pairs == 2) sg0[2] = sg0[1];
        (void)select_block_lanes_pal<M.bits, M.ch, M.pairs, TPB, true>(wqb, ln.tx, sg0, ln.pal, sh.pattern, tt);
    }
    for (int it = 0; it < iterations; it++) {
        ln.tx.fence();
        int32_t q[3][2][4];
        PalSegment sg[3];
        #pragma unroll
        for (int j = 0; j < M.pairs; j++) {
            float ep[2][4];
            int32_t d[2][4];
            ep[0][3] = 0.f; ep[1][3] = 0.f;
            refit_line<M.bits, M.ch>(ep, ln.tx.pl, wqb, sm[j], ln.T);
            quant_mode<MODE, false>(q[j], d, ep, settings_channels);       // :1343 passes the profile's channel count
            sg[j] = build_palette<M.bits, M.ch, TPB>(ln.pal + j * (LEVELS * TPB), d);
        }
        if (M.pairs == 2) sg[2] = sg[1];
        uint32_t qb[2];
        const int32_t err = select_block_lanes_pal<M.bits, M.ch, M.pairs, TPB, true>(qb, ln.tx, sg, ln.pal, sh.pattern, tt);
        const bool better = err < w.err;
        if (better) {
            #pragma unroll
            for (int j = 0; j < M.pairs; j++) for (int i = 0; i < 2; i++) for (int p = 0; p < 4; p++) cq[j][i][p] = q[j][i][p];
            wqb[0] = qb[0]; wqb[1] = qb[1];
            w.err = err;
        }
        // an iteration is a function of the kept indices alone (kernel.ispc:1331-1356): one that improves nothing leaves them
        // as they were, so every later one repeats it.  Once that holds for all 64 blocks of the wave the rest is skipped.
        if (__all(!better)) break;
    }
    int32_t err = w.err;
    if (MODE != 7) err += ln.opaque_err;
    if (err < ln.best_err) {
        ln.best_err = err;
        ln.improved = true;
        emit_multi<MODE>(ln.best, cq, wqb, w.shape);
    }
}

__device__ __forceinline__ void take(Win& w, int32_t err, int shape, int32_t key)
{
    w.err = err; w.shape = shape; w.key = key;
}

// modes 0 and 2: three subsets, every shape a candidate, one fit per subset.              [kernel.ispc:1386-1394]
// The reference scans the shapes in table order with a strict `<`: the winner is the lowest error and, among equal
// errors, the lowest table index -- whatever the visiting order.  With mode 2 enabled the scan therefore follows
// BC7_F02_SCHEDULE (tools/gen_bc7_f02_schedule.py): 192 (shape, subset) pairs use only 140 distinct texel masks and a
// subset's whole result under a mode (indices, error) depends on the mask alone, so the order clusters equal masks and
// two four-entry caches, driven by the wave-uniform schedule words, turn subset evaluations into loads: mode 2's over all
// 64 shapes (BC7_F02_SCHEDULE) and, with CACHE0, mode 0's over its 16 (BC7_F02_SCHEDULE_EXT).  A subset with every
// result it needs loaded is skipped outright -- moments, fit, both modes; one that loads a single mode keeps its fit.
// The counts are in the header's comment.  Without CACHE0 the primary word alone is run, a valid program by itself.
// A cached subset result is its error (the scans carry no indices).
// Mode 2's cache is four scalars (an indexed aggregate would be demoted to scratch); `slot` is wave-uniform.
// Mode 0's cache is four more words of the lane's LDS column, behind the twelve palette levels (pal[12 * TPB] and
// pal[13 * TPB]): the head scan has no register to spare, and a lane reads only what it wrote itself, so no barrier.
#define ITW_CACHE_GET(F, slot) ((slot) == 0u ? F##0 : ((slot) == 1u ? F##1 : ((slot) == 2u ? F##2 : F##3)))
#define ITW_CACHE_PUT(F, slot, v) do { F##0 = (slot) == 0u ? (v) : F##0; F##1 = (slot) == 1u ? (v) : F##1; F##2 = (slot) == 2u ? (v) : F##2; F##3 = (slot) == 3u ? (v) : F##3; } while (0)

// `first`/`step`: this call visits positions first, first + step, ... (the wide path splits one scan over several waves,
// WIDE below); a split scan takes the shapes in table order without the cache (any visiting order gives the same winner).
// CACHE0: the caller's LDS column has 14 levels.  SCHEDULED = false (test hook): table order, nothing cached.
// `trace` (test hook; null = none): the lane's per-shape errors, [0..15] mode 0 and [16..79] mode 2 by table index.
template <bool CACHE0 = false, bool SCHEDULED = true>
__device__ __forceinline__ void search_02(Lane& ln, const bc7_enc_settings& S, Win& b0, Win& b2, int first = 0, int step = 1, int32_t* trace = nullptr)
{
    reset(b0, 64); reset(b2, 64);
    IStats<3> full;
    stats_int<3>(full, ln.tx.pl, whole_block());
    const int32_t tt = full.m[0] + full.m[4] + full.m[7];          // sum over the block of |texel|^2
    const bool do2 = !S.skip_mode2;
    const int count = do2 ? 64 : 16;
    const bool scheduled = SCHEDULED && do2 && step == 1;            // mode 0 alone / split scan: table order, nothing cached
    int32_t ce0 = 0, ce1 = 0, ce2 = 0, ce3 = 0;      // cached subset results (mode 2 error of a texel mask)
    for (int pos = first; pos < count; pos += step) {
        ln.tx.fence();
        const uint32_t sched = scheduled ? BC7_F02_SCHEDULE[pos] : (uint32_t)pos;
        const uint32_t ext = (CACHE0 && scheduled) ? BC7_F02_SCHEDULE_EXT[pos] : 0u;
        const int part = (int)(sched & 63u);
        const bool do0 = part < 16;
        int32_t e0 = 0, e2 = 0;
        IStats<3> rest = full;
        bool rest_valid = true;                          // `rest` = block minus the subsets handled so far
        #pragma unroll 1
        for (int j = 0; j < 3; j++) {
            ln.tx.fence();                                // texel-derived values are used once per shape: do not hoist
            const uint32_t act = (sched >> (8 + 4 * j)) & 3u, slot = (sched >> (10 + 4 * j)) & 3u;
            const uint32_t act0 = (ext >> (4 * j)) & 3u, slot0 = (ext >> (4 * j + 2)) & 3u;
            int32_t* const c0 = reinterpret_cast<int32_t*>(ln.pal + (12u + (slot0 >> 1)) * TPB) + (slot0 & 1u);
            const bool load = act == 2u;                  // this mask's mode 2 result is in the cache
            const bool load0 = CACHE0 && act0 == 2u;      // and its mode 0 result
            if (load) e2 += ITW_CACHE_GET(ce, slot);
            if (load0) e0 += *c0;
            const bool need0 = do0 && !load0;
            if (load && !need0) { rest_valid = false; continue; }
            const SubsetMask sm = subset_of(64 + part, j);
            IStats<3> st;
            if (j < 2 || !rest_valid) stats_int<3>(st, ln.tx.pl, sm); else st = rest;
            stats_sub<3>(rest, st);
            float fit[2][4];
            fit[0][3] = 0.f; fit[1][3] = 0.f;            // the reference's unwritten alpha slots, pinned to 0
            fit_line<3>(fit, ln.tx, sm.bits, st, rcp_of_count(sm.n), ln.T);
            int32_t q[2][4], d[2][4];
            if (need0) {
                quant_mode<0, true>(q, d, fit, 3);
                const PalSegment ps = build_palette<3, 3, TPB>(ln.pal, d);
                int32_t r = 0;
                subset_error_pal<3, 3, TPB>(CACHE0 ? r : e0, ln.tx, ps, ln.pal, sm.bits);
                if (CACHE0) {
                    e0 += r;
                    if (act0 == 1u) *c0 = r;
                }
            }
            if (do2 && !load) {
                quant_mode<2, true>(q, d, fit, 3);
                const PalSegment ps = build_palette<2, 3, TPB>(ln.pal + 8 * TPB, d);
                int32_t r = 0;
                subset_error_pal<2, 3, TPB>(r, ln.tx, ps, ln.pal + 8 * TPB, sm.bits);
                e2 += r;
                if (act == 1u) ITW_CACHE_PUT(ce, slot, r);
            }
        }
        e0 += tt; e2 += tt;                              // the |t|^2 terms the palette path leaves out
        const int shape = 64 + part;
        if (do0 && (e0 < b0.err || (e0 == b0.err && shape < b0.shape))) take(b0, e0, shape, part);
        if (do2 && (e2 < b2.err || (e2 == b2.err && shape < b2.shape))) take(b2, e2, shape, part);
#ifdef ITW_TEST_HOOKS
        if (trace) { if (do0) trace[part] = e0; if (do2) trace[16 + part] = e2; }
#endif
    }
}

// Two-subset modes.  FAMILY7 = false: modes 1 and 3 (3-channel fit, shared);  true: mode 7 (4-channel fit).
// RANK_CH: channels used by the PCA ranking (3 for modes 1/3; the profile's channel count for mode 7).
// RANKED: 0 = every shape is a candidate (table-order scan); 1 = at least one of the family's lists is a proper prefix
// of the PCA ranking (fast profiles), keys in LDS; 2 = the same with lists of at most 16 shapes (every preset of the
// reference): the 16 smallest keys are kept sorted in registers while the keys are produced, no LDS.
// `first`/`step`: the share of a split scan (wide path): table-order scans visit shapes first, first + step, ...; ranked
// scans compute all 64 keys and evaluate list entries first, first + step, ...
template <bool FAMILY7, int RANK_CH, int RANKED>
__device__ __forceinline__ void search_two_subset(Lane& ln, const bc7_enc_settings& S, Win& wa, Win& wb, int first = 0, int step = 1)
{
    constexpr int FIT_CH = FAMILY7 ? 4 : 3;
    const int na = FAMILY7 ? S.fastSkipTreshold_mode7 : S.fastSkipTreshold_mode1;   // first mode of the family
    const int nb = FAMILY7 ? 0 : S.fastSkipTreshold_mode3;                           // second mode
    reset(wa, 0); reset(wb, 0);
    if (na <= 0 && nb <= 0) return;

    IStats<FIT_CH> full;
    stats_int<FIT_CH>(full, ln.tx.pl, whole_block());
    const int32_t tt = full.m[0] + full.m[4] + full.m[7] + (FIT_CH == 4 ? full.m[9] : 0);     // sum over the block of |texel|^2
    Stats<RANK_CH> rfull;                                 // the ranking's view of the block (first RANK_CH channels)
    {
        IStats<RANK_CH> t;
        #pragma unroll
        for (int i = 0; i < 10; i++) t.m[i] = full.m[i];
        #pragma unroll
        for (int i = 0; i < 4; i++) t.s[i] = full.s[i];
        t.n = 16;
        stats_float<RANK_CH>(rfull, t);
    }

    if (RANKED == 0) {
        // every shape is a candidate: table order; the rank key is only needed to order shapes of equal error
        for (int part = first; part < 64; part += step) {
            ln.tx.fence();
            int32_t ea = 0, ec = 0;
            IStats<FIT_CH> rest = full;
            #pragma unroll 1
            for (int j = 0; j < 2; j++) {
                ln.tx.fence();                            // texel-derived values are used once per shape: do not hoist
                const SubsetMask sm = subset_of(part, j);
                IStats<FIT_CH> st;
                if (j == 0) stats_int<FIT_CH>(st, ln.tx.pl, sm); else st = rest;
                stats_sub<FIT_CH>(rest, st);
                float fit[2][4];
                fit[0][3] = 0.f; fit[1][3] = 0.f;
                fit_line<FIT_CH>(fit, ln.tx, sm.bits, st, rcp_of_count(sm.n), ln.T);
                int32_t q[2][4], d[2][4];
                if (FAMILY7) {
                    quant_mode<7, true>(q, d, fit, 4);
                    const PalSegment ps = build_palette<2, 4, TPB>(ln.pal, d);
                    subset_error_pal<2, 4, TPB>(ea, ln.tx, ps, ln.pal, sm.bits);
                } else {
                    if (na > 0 && nb > 0) {
                        quant_mode<1, true>(q, d, fit, 3);
                        const PalSegment s1 = build_palette<3, 3, TPB>(ln.pal, d);
                        quant_mode<3, true>(q, d, fit, 3);
                        const PalSegment s3 = build_palette<2, 3, TPB>(ln.pal + 8 * TPB, d);
                        subset_error2_pal<3, 2, 3, TPB>(ea, ec, ln.tx, s1, ln.pal, s3, ln.pal + 8 * TPB, sm.bits);
                    } else if (na > 0) {
                        quant_mode<1, true>(q, d, fit, 3);
                        const PalSegment ps = build_palette<3, 3, TPB>(ln.pal, d);
                        subset_error_pal<3, 3, TPB>(ea, ln.tx, ps, ln.pal, sm.bits);
                    } else {
                        quant_mode<3, true>(q, d, fit, 3);
                        const PalSegment ps = build_palette<2, 3, TPB>(ln.pal + 8 * TPB, d);
                        subset_error_pal<2, 3, TPB>(ec, ln.tx, ps, ln.pal + 8 * TPB, sm.bits);
                    }
                }
            }
            ea += tt; ec += tt;                          // the |t|^2 terms the palette path leaves out
            const bool on_a = na > 0, on_b = !FAMILY7 && nb > 0;
            const bool tie_a = on_a && ea == wa.err, tie_b = on_b && ec == wb.err;
            if (on_a && ea < wa.err) take(wa, ea, part, -1);
            if (on_b && ec < wb.err) take(wb, ec, part, -1);
            if (tie_a || tie_b) {
                // equal errors: the reference keeps whichever comes first in its ranked list = the lower key.
                // One rolled loop evaluates the missing keys: this shape's, then the incumbents'.
                int32_t key_here = 0;
                #pragma unroll 1
                for (int which = 0; which < 3; which++) {
                    const int shape = (which == 0) ? part : ((which == 1) ? wa.shape : wb.shape);
                    const bool need = (which == 0) || (which == 1 && tie_a && wa.key < 0) || (which == 2 && tie_b && wb.key < 0);
                    if (need) {
                        const int32_t k = rank_key<RANK_CH>(shape, ln.tx, rfull, ln.T);
                        if (which == 0) key_here = k; else if (which == 1) wa.key = k; else wb.key = k;
                    }
                }
                if (tie_a && key_here < wa.key) take(wa, ea, part, key_here);
                if (tie_b && key_here < wb.key) take(wb, ec, part, key_here);
            }
        }
    } else {
        // ranked prefix: the i-th list entry of the reference's selection sort is the i-th smallest key (keys are
        // distinct: their low 6 bits are the shape)                                      [kernel.ispc:1400-1414]
        int32_t top[16];
        #pragma unroll
        for (int i = 0; i < 16; i++) top[i] = 0x7fffffff;
        const int nlist = min(max(na, nb), 16);                   // entries of the ranked list that will be read (wave-uniform)
        for (int part = 0; part < 64; part++) {
            ln.tx.fence();
            const int32_t key = rank_key<RANK_CH>(part, ln.tx, rfull, ln.T);
            if (RANKED == 1) {
                ln.keys[part * TPB] = key;
            } else {
                // sorted insertion into the `nlist` smallest keys seen so far: a chain of compare-exchanges as long as the list the settings ask
                // for, in steps of four (wave-uniform: three scalar branches; `veryfast` keeps 3 keys, not 16: 24 of 32 VALU per shape saved)
                int32_t x = key;
#define ITW_INS4(b) { _Pragma("unroll") for (int i = (b); i < (b) + 4; i++) { const int32_t lo = min(top[i], x); x = max(top[i], x); top[i] = lo; } }
                ITW_INS4(0)
                if (nlist > 4) { ITW_INS4(4) if (nlist > 8) { ITW_INS4(8) if (nlist > 12) ITW_INS4(12) } }
#undef ITW_INS4
            }
        }
        const int n = min(max(na, nb), RANKED == 1 ? 64 : 16);
        int32_t prev = 0;
        for (int i = 0; i < n; i++) {
            if (RANKED == 1) {
                int32_t cur = 0x7fffffff;
                for (int t = 0; t < 64; t++) {
                    const int32_t k = ln.keys[t * TPB];
                    if ((i == 0 || k > prev) && k <= cur) cur = k;
                }
                prev = cur;
            } else {
                prev = top[0];
                #pragma unroll
                for (int t = 0; t < 15; t++) top[t] = top[t + 1];
            }
            if (step > 1 && (i % step) != first) continue;       // another wave's share of the list
            ln.tx.fence();
            const int shape = prev & 63;
            const Shape sh = load_shape(shape);
            if (RANKED == 2) {
                // lists of at most 16 shapes (every preset): the candidate's subsets decode their palettes into the lane's LDS column
                // (mode 1: 2 x 8 levels; mode 3 afterwards over the same stretch: 2 x 4) and the texels are scored through them
                float fits[2][2][4];
                IStats<FIT_CH> rest2 = full;
                #pragma unroll
                for (int j = 0; j < 2; j++) {
                    const SubsetMask sm = subset_of(shape, j);
                    IStats<FIT_CH> st;
                    if (j == 0) stats_int<FIT_CH>(st, ln.tx.pl, sm); else st = rest2;
                    stats_sub<FIT_CH>(rest2, st);
                    fits[j][0][3] = 0.f; fits[j][1][3] = 0.f;
                    fit_line<FIT_CH>(fits[j], ln.tx, sm.bits, st, ispc_rcp((float)sm.n, ln.T), ln.T);
                }
                uint32_t qbl[2];
                int32_t q[2][4], d[2][4];
                PalSegment ps[3];
                if (FAMILY7) {
                    #pragma unroll
                    for (int j = 0; j < 2; j++) { quant_mode<7, true>(q, d, fits[j], 4); ps[j] = build_palette<2, 4, TPB>(ln.pal + j * (4 * TPB), d); }
                    ps[2] = ps[1];
                    const int32_t e = select_block_lanes_pal<2, 4, 2, TPB, false>(qbl, ln.tx, ps, ln.pal, sh.pattern, tt);
                    if (e < wa.err) take(wa, e, shape, prev);
                } else {
                    if (i < na) {
                        #pragma unroll
                        for (int j = 0; j < 2; j++) { quant_mode<1, true>(q, d, fits[j], 3); ps[j] = build_palette<3, 3, TPB>(ln.pal + j * (8 * TPB), d); }
                        ps[2] = ps[1];
                        const int32_t e = select_block_lanes_pal<3, 3, 2, TPB, false>(qbl, ln.tx, ps, ln.pal, sh.pattern, tt);
                        if (e < wa.err) take(wa, e, shape, prev);
                    }
                    if (i < nb) {
                        #pragma unroll
                        for (int j = 0; j < 2; j++) { quant_mode<3, true>(q, d, fits[j], 3); ps[j] = build_palette<2, 3, TPB>(ln.pal + j * (4 * TPB), d); }
                        ps[2] = ps[1];
                        const int32_t e = select_block_lanes_pal<2, 3, 2, TPB, false>(qbl, ln.tx, ps, ln.pal, sh.pattern, tt);
                        if (e < wb.err) take(wb, e, shape, prev);
                    }
                }
                continue;
            }
            Segment sa[3], sc[3];
            IStats<FIT_CH> rest = full;
            #pragma unroll
            for (int j = 0; j < 2; j++) {
                const SubsetMask sm = subset_of(shape, j);
                IStats<FIT_CH> st;
                if (j == 0) stats_int<FIT_CH>(st, ln.tx.pl, sm); else st = rest;
                stats_sub<FIT_CH>(rest, st);
                float fit[2][4];
                fit[0][3] = 0.f; fit[1][3] = 0.f;
                fit_line<FIT_CH>(fit, ln.tx, sm.bits, st, ispc_rcp((float)sm.n, ln.T), ln.T);
                int32_t q[2][4], d[2][4];
                if (FAMILY7) {
                    quant_mode<7, true>(q, d, fit, 4);
                    sa[j] = make_segment<2, 4>(d);
                } else {
                    quant_mode<1, true>(q, d, fit, 3);
                    sa[j] = make_segment<3, 3>(d);
                    quant_mode<3, true>(q, d, fit, 3);
                    sc[j] = make_segment<2, 3>(d);
                }
            }
            sa[2] = sa[1]; sc[2] = sc[1];
            uint32_t qb[2];
            if (FAMILY7) {
                const int32_t e = select_block<2, 4, 2>(qb, ln.tx, sa, sh.pattern);
                if (e < wa.err) take(wa, e, shape, prev);
            } else {
                if (i < na) {
                    const int32_t e = select_block<3, 3, 2>(qb, ln.tx, sa, sh.pattern);
                    if (e < wa.err) take(wa, e, shape, prev);
                }
                if (i < nb) {
                    const int32_t e = select_block<2, 3, 2>(qb, ln.tx, sc, sh.pattern);
                    if (e < wb.err) take(wb, e, shape, prev);
                }
            }
        }
    }
}

// ---- modes 4 and 5: vector part (3 channels) + one separately coded channel ------------------

template <int BITS>
__device__ __forceinline__ int32_t weight_single(int32_t q)                       // kernel.ispc:675-686
{
    if (BITS == 2) return (int32_t)__builtin_amdgcn_perm(0u, 0x402b1500u, (uint32_t)q | 0x0c0c0c00u);
    if (BITS == 3) return (int32_t)__builtin_amdgcn_perm(0x40372e25u, 0x1b120900u, (uint32_t)q | 0x0c0c0c00u);
    return (int32_t)(((uint32_t)q * 68u + 8u) >> 4);
}

// scalar channel: min/max endpoints, then `iters` rounds of LS refit.             [kernel.ispc:1437-1563]
// Values v are the block's bytes of channel `rot_ch` (16 integers); vp = the same channel in planar form.
// Integer-exact parts: decode (int)(((64-w)*e0 + w*e1 + 32)/64) = e0 + ((w*(e1-e0)+32) >> 6), squared errors,
// and all sums of channel_opt_endpoints (<= 16*15*255).  The projection keeps the reference's fp32 form:
// (v - e0) is exact, * rcp(e1 - e0 + 0.001f), * LEVELS (exact) + 0.5 (one FMA = two roundings here).
// The LEVELS decoded values of a round are written once to the lane's own palette column in LDS and a texel reads its two
// neighbouring levels: two weights, two multiplies and six integer adds/shifts per texel become one address and one read.
template <int BITS, int EPBITS>
__device__ __forceinline__ int32_t encode_scalar(uint32_t (&qb)[2], int32_t (&qe)[2], const Tex& tx, int rot_ch,
                                                 const uint32_t (&vp)[4], int iters, const SeedTables& T, uint2* lv)
{
    constexpr int LEVELS = 1 << BITS;
    constexpr uint32_t LM1 = LEVELS - 1;
    constexpr float L1 = (float)LM1;
    constexpr int EL = 1 << EPBITS;
    const uint32_t shift = 8u * (uint32_t)rot_ch;
    int32_t lo = 255, hi = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) { const int32_t v = (int32_t)((tx.w[k] >> shift) & 255u); lo = min(lo, v); hi = max(hi, v); }
    float ep[2] = {(float)lo, (float)hi};
    int32_t err = 0;
    uint32_t pqb0 = 0, pqb1 = 0;
    for (int round = 0; ; round++) {
        int32_t de[2];
        #pragma unroll
        for (int i = 0; i < 2; i++) {                                            // channel_quant_dequant
            qe[i] = iclamp((int32_t)(ep[i] * INV255 * (float)(EL - 1) + 0.5f), 0, EL - 1);   // ep in [0,255]
            de[i] = expand_to_byte(qe[i], EPBITS);
        }
        qb[0] = qb[1] = 0u;                                                      // channel_opt_quant
        err = 0;
        const int32_t span = de[1] - de[0];
        const float rspan = ispc_rcp((float)span + 0.001f, T);
        // entry l of the lane's own palette column holds the float bits of levels (l, l + 1): one 8-byte read per texel
        // (the column is the vector palette's, dead by now; same element type, so no type-based reordering against the
        // next candidate's palette stores; other lanes' entries belong to waves that may be anywhere)
        {
            float lvl[LEVELS];
#pragma unroll
            for (int l = 0; l < LEVELS; l++) {
                constexpr int D = LEVELS - 1;
                const int32_t w = (l * 128 + D) / (2 * D);                       // the format's weight of level l (compile time)
                lvl[l] = (float)((l == 0) ? de[0] : (l == D) ? de[1] : de[0] + ((w * span + 32) >> 6));
            }
#pragma unroll
            for (int l = 0; l + 1 < LEVELS; l++) lv[l * TPB] = make_uint2(__float_as_uint(lvl[l]), __float_as_uint(lvl[l + 1]));
        }
        // texel values, decoded levels and their differences are integers below 2^8, squares and their sum stay below
        // 2^24: the float forms below are exact, and fp32 mul / sub issue at twice the rate of the integer multiply
        const float de0f = (float)de[0];
        float errf = 0.f;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            // planar words hold texels {0,2,4,6} {1,3,5,7} {8,10,12,14} {9,11,13,15}: one v_cvt_f32_ubyteN each
            const float vf = (float)((vp[(k >> 3) * 2 + (k & 1)] >> (8 * ((k & 7) >> 1))) & 255u);
            const float proj = (vf - de0f) * rspan;                              // (float)(v - de0) of the reference, exact
            const int32_t q1 = imed3((int32_t)__builtin_fmaf(proj, (float)LEVELS, 0.5f), 1, LEVELS - 1);
            const uint2 pr = lv[(q1 - 1) * TPB];
            const float x0 = __uint_as_float(pr.x) - vf, x1 = __uint_as_float(pr.y) - vf;
            const float e0 = x0 * x0, e1 = x1 * x1;
            const bool first = e0 < e1;
            const uint32_t q = (uint32_t)(first ? q1 - 1 : q1);
            if (k < 8) qb[0] |= q << (4 * k); else qb[1] |= q << (4 * (k - 8));
            errf += __builtin_fminf(e0, e1);
        }
        err = (int32_t)errf;
        if (round >= iters) break;
        // the next round's endpoints are a function of these indices (channel_opt_endpoints): if they repeat the previous
        // round's for every block of the wave, all further rounds repeat this one
        if (__all(round > 0 && qb[0] == pqb0 && qb[1] == pqb1)) break;
        pqb0 = qb[0]; pqb1 = qb[1];
        const uint32_t qn[4] = {qb[0] & 0x0f0f0f0fu, (qb[0] >> 4) & 0x0f0f0f0fu, qb[1] & 0x0f0f0f0fu, (qb[1] >> 4) & 0x0f0f0f0fu};
        uint32_t sq_ = 0, sqq = 0, ssum = 0, satb = 0;                           // channel_opt_endpoints
#pragma unroll
        for (int d = 0; d < 4; d++) {
            sq_ = udot4(qn[d], 0x01010101u, sq_);
            sqq = udot4(qn[d], qn[d], sqq);
            ssum = udot4(vp[d], 0x01010101u, ssum);
            satb = udot4(vp[d], LM1 * 0x01010101u - qn[d], satb);
        }
        const float sum_q = (float)sq_, sum_qq = (float)sqq, sum = (float)ssum, atb1 = (float)satb;
        const float atb2 = L1 * sum - atb1;
        const float cxx = 16.0f * (L1 * L1) - (2.0f * L1) * sum_q + sum_qq;
        const float cyy = sum_qq;
        const float cxy = L1 * sum_q - sum_qq;
        const float det = cxx * cyy - cxy * cxy;
        const float scale = L1 * ispc_rcp(det, T);
        ep[0] = fclamp_num((atb1 * cyy - atb2 * cxy) * scale, 0.f, 255.f);
        ep[1] = fclamp_num((atb2 * cxx - atb1 * cxy) * scale, 0.f, 255.f);
        if (fabsf(det) < 0.001f) { ep[0] = sum * 0.0625f; ep[1] = ep[0]; }
    }
    return err;
}

// one (mode, rotation, index-swap) candidate, given the rotation's line fit      [kernel.ispc:1565-1621]
// `bound`: an error this candidate must stay below to matter at all (<= best_err).  The candidate's error is its vector part's plus
// its scalar channel's (>= 0) and it is taken only on a strict `<`: where the vector part alone reaches the bound for all 64
// blocks of the wave, the scalar channel (up to refineIterations_channel + 1 rounds over the 16 texels) is not encoded.
template <int MODE, int SWAP>
__device__ __forceinline__ void try_dual(Dual& best, int32_t& best_err, int32_t bound, const Lane& ln, Tex& rot, const float (&fit)[2][4], int32_t tt,
                                         const bc7_enc_settings& S, int rotation)
{
    constexpr int BITS = SWAP ? 3 : 2;
    constexpr int ABITS = SWAP ? 2 : ((MODE == 4) ? 3 : 2);
    constexpr int AEPB = (MODE == 4) ? 6 : 8;
    const SubsetMask all = whole_block();
    rot.fence();                                    // values derived from the rotated texels must not stay live across candidates

    int32_t q[2][4], d[2][4];
    uint32_t qb[2];
    quant_mode<MODE, true>(q, d, fit, 3);
    PalSegment ps = build_palette<BITS, 3, TPB>(ln.pal, d);
    int32_t err = select_block_pal<BITS, 3, TPB>(qb, rot, ps, ln.pal, tt);
    const int iters = S.refineIterations[MODE];
    for (int it = 0; it < iters; it++) {
        float ep[2][4];
        ep[0][3] = 0.f; ep[1][3] = 0.f;
        const uint32_t was0 = qb[0], was1 = qb[1];
        refit_line<BITS, 3>(ep, rot.pl, qb, all, ln.T);
        quant_mode<MODE, false>(q, d, ep, 3);
        ps = build_palette<BITS, 3, TPB>(ln.pal, d);
        err = select_block_pal<BITS, 3, TPB>(qb, rot, ps, ln.pal, tt);
        // the iteration maps indices to (endpoints, indices, error) (kernel.ispc:1598-1603): unchanged indices are a fixed
        // point, further iterations reproduce exactly these values
        if (__all(qb[0] == was0 && qb[1] == was1)) break;
    }

    if (__all(err >= bound)) return;

    int32_t aq[2];
    uint32_t aqb[2];
    const uint32_t vp[4] = {ln.tx.pl[0][0], ln.tx.pl[0][1], ln.tx.pl[0][2], ln.tx.pl[0][3]};
    const uint32_t vg[4] = {ln.tx.pl[1][0], ln.tx.pl[1][1], ln.tx.pl[1][2], ln.tx.pl[1][3]};
    const uint32_t vb[4] = {ln.tx.pl[2][0], ln.tx.pl[2][1], ln.tx.pl[2][2], ln.tx.pl[2][3]};
    const uint32_t va[4] = {ln.tx.pl[3][0], ln.tx.pl[3][1], ln.tx.pl[3][2], ln.tx.pl[3][3]};
    uint32_t vsel[4];
    #pragma unroll
    for (int i = 0; i < 4; i++) vsel[i] = (rotation == 0) ? vp[i] : ((rotation == 1) ? vg[i] : ((rotation == 2) ? vb[i] : va[i]));
    err += encode_scalar<ABITS, AEPB>(aqb, aq, ln.tx, rotation, vsel, S.refineIterations_channel, ln.T, ln.pal);

    if (err < best_err) {
        #pragma unroll
        for (int i = 0; i < 2; i++) for (int p = 0; p < 4; p++) best.q[i][p] = q[i][p];
        best.qb[0] = qb[0]; best.qb[1] = qb[1];
        best.aq[0] = aq[0]; best.aq[1] = aq[1];
        best.aqb[0] = aqb[0]; best.aqb[1] = aqb[1];
        best.rotation = rotation;
        best.swap = SWAP;
        best_err = err;
    }
}

__device__ __forceinline__ void clear(Dual& d)
{
    #pragma unroll
    for (int i = 0; i < 2; i++) for (int p = 0; p < 4; p++) d.q[i][p] = 0;
    d.qb[0] = d.qb[1] = d.aqb[0] = d.aqb[1] = 0u;
    d.aq[0] = d.aq[1] = 0; d.rotation = 0; d.swap = 0;
}

// The reference tries all mode 4 candidates (rotation-major, swap-minor), commits, then all mode 5 candidates.
// Here one pass over the rotations serves both: a rotation's line fit does not depend on the mode.  Mode 5's
// winner is found independently (first strict minimum in rotation order) and admitted afterwards against the
// error left by mode 4 -- the same block the sequential scan produces.
// Rotations r0 .. r1-1 (the wide path gives each rotation its own wave).
// `which`: bit 0 = mode 4 without index swap, bit 1 = mode 4 swapped, bit 2 = mode 5 (the wide path runs them as separate tasks).
__device__ __forceinline__ void modes_45_scan(Lane& ln, const bc7_enc_settings& S, int r0, int r1, Dual& best4, int32_t& err4, Dual& best5, int32_t& err5,
                                              int which = 7)
{
    for (int r = r0; r < r1; r++) {
        // rotated colour block: channel r is replaced by alpha (RGBA profile) or 255 (RGB profile);
        // the displaced channel is coded separately
        Tex rot;
        const uint32_t sh8 = 8u * (uint32_t)r;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const uint32_t w = ln.tx.w[k];
            uint32_t v = w;
            if (r < 3) {
                const uint32_t fill = (S.channels == 4) ? (w >> 24) : 255u;
                v = (w & ~(255u << sh8)) | (fill << sh8);
            }
            rot.w[k] = v;
        }
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int d = 0; d < 4; d++) {
                const uint32_t fill = (S.channels == 4) ? ln.tx.pl[3][d] : 0xffffffffu;
                rot.pl[c][d] = (c == r && r < 3) ? fill : ln.tx.pl[c][d];
            }
        IStats<3> st;
        stats_int<3>(st, rot.pl, whole_block());
        float fit[2][4];
        fit[0][3] = 0.f; fit[1][3] = 0.f;
        fit_line<3>(fit, rot, 0xffffu, st, rcp_of_count(16), ln.T);
        const int32_t tt = st.m[0] + st.m[4] + st.m[7];          // |texel|^2 summed over the rotated colour block
        if (which & 1) try_dual<4, 0>(best4, err4, err4, ln, rot, fit, tt, S, r);
        if (which & 2) try_dual<4, 1>(best4, err4, err4, ln, rot, fit, tt, S, r);
        // mode 5's winner is admitted only below the error mode 4 leaves (modes_45; the wide path's commit order), and err4 only
        // falls from here on: a mode 5 candidate at or above it can neither be admitted nor hide one that could
        if (which & 4) try_dual<5, 0>(best5, err5, min(err5, err4), ln, rot, fit, tt, S, r);
    }
}

__device__ __forceinline__ void modes_45(Lane& ln, const bc7_enc_settings& S)      // [kernel.ispc:1623-1655]
{
    Dual best4, best5;
    clear(best4); clear(best5);
    int32_t err4 = ln.best_err, err5 = ERR_MAX;
    modes_45_scan(ln, S, S.mode45_channel0, S.channels, best4, err4, best5, err5);
    if (err4 < ln.best_err) { ln.best_err = err4; ln.improved = true; emit_dual<4>(ln.best, best4); }
    if (err5 < ln.best_err) { ln.best_err = err5; ln.improved = true; emit_dual<5>(ln.best, best5); }
}

// ---- mode 6: one subset, RGBA, 4-bit indices                                     [kernel.ispc:1657-1689]
template <int CH>
__device__ __forceinline__ void mode_6(Lane& ln, const bc7_enc_settings& S)
{
    const SubsetMask all = whole_block();
    IStats<CH> st;
    stats_int<CH>(st, ln.tx.pl, all);
    float ep[2][4];
    int32_t q[2][4], d[2][4];
    uint32_t qb[2];
    Segment sg[3];
    ep[0][3] = 0.f; ep[1][3] = 0.f;
    fit_line<CH>(ep, ln.tx, 0xffffu, st, rcp_of_count(16), ln.T);
    if (CH == 3) { ep[0][3] = 255.f; ep[1][3] = 255.f; }
    quant_mode<6, true>(q, d, ep, CH);
    // the sixteen decoded colours once into the lane's LDS column, then one projection, one 16-byte read and two dot products
    // per texel instead of decoding both neighbouring levels with packed 16-bit math per texel (bc7_exact.hpp)
    const int32_t tt = block_norm2<CH>(ln.tx.pl);
    PalSegment ps = build_palette<4, CH, TPB>(ln.pal, d);
    int32_t err = select_block_pal<4, CH, TPB>(qb, ln.tx, ps, ln.pal, tt);
    (void)sg;
    const int iters = S.refineIterations[6];
    for (int it = 0; it < iters; it++) {
        const uint32_t was0 = qb[0], was1 = qb[1];
        refit_line<4, CH>(ep, ln.tx.pl, qb, all, ln.T);
        quant_mode<6, false>(q, d, ep, CH);
        ps = build_palette<4, CH, TPB>(ln.pal, d);
        err = select_block_pal<4, CH, TPB>(qb, ln.tx, ps, ln.pal, tt);
        if (__all(qb[0] == was0 && qb[1] == was1)) break;         // fixed point of the iteration (kernel.ispc:1672-1677)
    }
    if (err < ln.best_err) {
        ln.best_err = err;
        ln.improved = true;
        emit_mode6(ln.best, q, qb);
    }
}

// ---- kernels ----------------------------------------------------------------------------------------
// Per multi-subset family two kernels: SEARCH (scan of the shapes; low register pressure, runs at 3-4 waves per SIMD)
// leaves each mode's winner {indices, error, shape} in the workspace, FINISH refines the winners and lets them compete
// for the block.  Modes 4/5/6 are one kernel.  Splitting keeps the register allocation of the scan independent of the
// (per-lane shape, fully unrolled) refinement code.
template <bool VEC16>
__device__ __forceinline__ void load_block(Tex& tx, const uint8_t* __restrict__ src, int64_t stride, int32_t blocks_x, int32_t b)
{
    const int32_t yy = b / blocks_x, xx = b - yy * blocks_x;
    const uint8_t* p = src + (int64_t)yy * 4 * stride + (int64_t)xx * 16;
#pragma unroll
    for (int y = 0; y < 4; y++) {
        if (VEC16) {
            const uint4 v = *reinterpret_cast<const uint4*>(p + y * stride);
            tx.w[y * 4 + 0] = v.x; tx.w[y * 4 + 1] = v.y; tx.w[y * 4 + 2] = v.z; tx.w[y * 4 + 3] = v.w;
        } else {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(p + y * stride);
            #pragma unroll
            for (int x = 0; x < 4; x++) tx.w[y * 4 + x] = q[x];
        }
    }
    tx.make_planar();
}

// Round 5: the blocks a finish phase lists for a later scan also leave their 64 B of texels in a compact buffer, in list order, so the
// list scans (up to 8 shares per block) and their refinement read contiguous lines instead of gathering 64 B out of every 128 B line
__device__ __forceinline__ void load_block_compact(Tex& tx, const uint4* __restrict__ compact, int32_t slot)
{
    const uint4* p = compact + (int64_t)slot * 4;
#pragma unroll
    for (int y = 0; y < 4; y++) { const uint4 v = p[y]; tx.w[y * 4 + 0] = v.x; tx.w[y * 4 + 1] = v.y; tx.w[y * 4 + 2] = v.z; tx.w[y * 4 + 3] = v.w; }
    tx.make_planar();
}

// winners of a family's two modes: [slot][block] x {err, shape}  (8 B; the workspace keeps its 16 B slots)
__device__ __forceinline__ void store_win(uint4* __restrict__ wins, int32_t nblocks, int slot, int32_t b, const Win& w)
{
    reinterpret_cast<uint2*>(wins)[(int64_t)slot * nblocks + b] = make_uint2((uint32_t)w.err, (uint32_t)w.shape);
}
__device__ __forceinline__ void load_win(Win& w, const uint4* __restrict__ wins, int32_t nblocks, int slot, int32_t b)
{
    const uint2 v = reinterpret_cast<const uint2*>(wins)[(int64_t)slot * nblocks + b];
    w.err = (int32_t)v.x; w.shape = (int32_t)v.y; w.key = -1;
}

// Register budgets (waves per SIMD) were picked by measurement on MI355X: the scans are bound by dependent-issue
// and LDS latency at 2 waves, and tolerate a few spilled cold values to reach 3-4.  Re-swept in round 6 under the max-ILP schedule
// (profiles/r06_rejected_experiments.txt, item 10): only the unranked mode 7 scan moved, 3 -> 4 (alpha_slow -3...-5 %).
#ifndef SW02
#define SW02 4
#endif
#ifndef SW13
#define SW13 4
#endif
#ifndef SWALL
#define SWALL 4
#endif
#ifndef SW7
#define SW7 4
#endif
#ifndef SWR
#define SWR 2
#endif
#ifndef SWR2
#define SWR2 3
#endif
#ifndef SWR27
#define SWR27 2
#endif
#ifndef FW
#define FW 3
#endif
#ifndef FW456
#define FW456 2
#endif
__host__ __device__ constexpr int search_waves(int family, int ranked) { return ranked == 2 ? (family == F_MODE7 ? SWR27 : SWR2) : ranked ? SWR : (family == F_MODE7 ? SW7 : (family == F_MODES02 ? SW02 : SW13)); }
__host__ __device__ constexpr int finish_waves(int family) { return family == F_MODES13 ? FW : FW456; }

template <int FAMILY, int RANKED, bool VEC16>
__global__ void __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(search_waves(FAMILY, RANKED), search_waves(FAMILY, RANKED))))
bc7_search_kernel(const uint8_t* __restrict__ src, int64_t stride, int32_t blocks_x, int32_t nblocks,
                  uint4* __restrict__ wins, const bc7_enc_settings S)
{
    __shared__ unsigned short s_seed16[2048];
    __shared__ uint32_t s_seed32[2048];
    extern __shared__ int32_t s_keys[];            // 64 * TPB keys, only allocated for RANKED == 1
    // per-lane palettes: table-order scans 8 + 4 levels (24 KiB); ranked lists <= 16: 2 subsets x 8 levels (32 KiB); longer lists: none
    __shared__ uint2 s_pal[RANKED == 0 ? 12 * TPB : RANKED == 2 ? 16 * TPB : 1];
    Lane ln;
    ln.T = stage_seed_tables_fast(s_seed16, s_seed32, threadIdx.x, TPB);
    __syncthreads();
    const int32_t gid = blockIdx.x * TPB + threadIdx.x;
    const bool live = gid < nblocks;
    const int32_t b = live ? gid : nblocks - 1;    // idle lanes of the last workgroup redo its last block, store nothing
    ln.keys = s_keys + threadIdx.x;
    ln.pal = s_pal + ((RANKED == 0 || RANKED == 2) ? threadIdx.x : 0);
    load_block<VEC16>(ln.tx, src, stride, blocks_x, b);

    Win wa, wb;
    if (FAMILY == F_MODES02) search_02(ln, S, wa, wb);
    if (FAMILY == F_MODES13) search_two_subset<false, 3, RANKED>(ln, S, wa, wb);
    if (FAMILY == F_MODE7) {
        if (S.channels == 4) search_two_subset<true, 4, RANKED>(ln, S, wa, wb); else search_two_subset<true, 3, RANKED>(ln, S, wa, wb);
    }
    if (live) {
        store_win(wins, nblocks, 0, b, wa);
        if (FAMILY != F_MODE7) store_win(wins, nblocks, 1, b, wb);
    }
}

template <int FAMILY, bool VEC16>
__global__ void __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(finish_waves(FAMILY), finish_waves(FAMILY))))
bc7_finish_kernel(const uint8_t* __restrict__ src, int64_t stride, int32_t blocks_x, int32_t nblocks,
                  uint8_t* __restrict__ dst, int32_t* __restrict__ err_ws, const uint4* __restrict__ wins,
                  const bc7_enc_settings S, const int first)
{
    __shared__ unsigned short s_seed16[2048];
    __shared__ uint32_t s_seed32[2048];
    // mode 4/5 vector part: one palette per lane (16 KiB); refinement of a family's winners: one per subset (pairs x levels)
    __shared__ uint2 s_pal[(FAMILY == F_MODES02 ? 24 : 16) * TPB];
    Lane ln;
    ln.T = stage_seed_tables_fast(s_seed16, s_seed32, threadIdx.x, TPB);
    __syncthreads();
    const int32_t gid = blockIdx.x * TPB + threadIdx.x;
    const bool live = gid < nblocks;
    const int32_t b = live ? gid : nblocks - 1;
    ln.keys = nullptr;
    ln.pal = s_pal + threadIdx.x;
    load_block<VEC16>(ln.tx, src, stride, blocks_x, b);

    ln.best_err = first ? ERR_MAX : err_ws[b];
    ln.best[0] = ln.best[1] = ln.best[2] = ln.best[3] = 0u;
    ln.improved = (first != 0);                    // the first family always defines the block
    ln.opaque_err = 0;                                                             // kernel.ispc:1267-1277
    if (S.channels == 4) {
        uint32_t e = 0;
#pragma unroll
        for (int d = 0; d < 4; d++) { const uint32_t x = ~ln.tx.pl[3][d]; e = udot4(x, x, e); }   // (255 - a)^2, bytewise
        ln.opaque_err = (int32_t)e;
    }

    if (FAMILY == F_MODES02) {
        Win w;
        load_win(w, wins, nblocks, 0, b);
        refine_and_commit<0>(ln, w, S.refineIterations[0], S.channels);
        if (!S.skip_mode2) { load_win(w, wins, nblocks, 1, b); refine_and_commit<2>(ln, w, S.refineIterations[2], S.channels); }
    }
    if (FAMILY == F_MODES13) {
        Win w;
        if (S.fastSkipTreshold_mode1 > 0) { load_win(w, wins, nblocks, 0, b); refine_and_commit<1>(ln, w, S.refineIterations[1], S.channels); }
        if (S.fastSkipTreshold_mode3 > 0) { load_win(w, wins, nblocks, 1, b); refine_and_commit<3>(ln, w, S.refineIterations[3], S.channels); }
    }
    if (FAMILY == F_MODE7) {
        Win w;
        load_win(w, wins, nblocks, 0, b);
        refine_and_commit<7>(ln, w, S.refineIterations[7], S.channels);
    }
    if (FAMILY == F_MODES456) {
        if (S.mode_selection[2]) modes_45(ln, S);
        if (S.mode_selection[3]) { if (S.channels == 4) mode_6<4>(ln, S); else mode_6<3>(ln, S); }
    }

    if (live && ln.improved) {
        uint32_t* d = reinterpret_cast<uint32_t*>(dst + (int64_t)b * 16);
        if (VEC16) *reinterpret_cast<uint4*>(d) = make_uint4(ln.best[0], ln.best[1], ln.best[2], ln.best[3]);
        else { d[0] = ln.best[0]; d[1] = ln.best[1]; d[2] = ln.best[2]; d[3] = ln.best[3]; }
        err_ws[b] = ln.best_err;
    }
}

enum WideKind { WK_SCAN02 = 0, WK_SCAN13 = 1, WK_SCAN7 = 2 };          // scan tasks of the fused and the wide path
__host__ __device__ constexpr int wide_win_slot(int mode) { return mode == 0 ? 0 : mode == 2 ? 1 : mode == 1 ? 2 : mode == 3 ? 3 : 4; }   // winner rows: m0 m2 m1 m3 m7

// the ranking's view of the whole block, for rank keys evaluated at merge time (same construction as search_two_subset)
template <int FIT_CH, int RANK_CH>
__device__ __forceinline__ void whole_block_rank_stats(Stats<RANK_CH>& rfull, const Tex& tx)
{
    IStats<FIT_CH> full;
    stats_int<FIT_CH>(full, tx.pl, whole_block());
    IStats<RANK_CH> t;
    #pragma unroll
    for (int i = 0; i < 10; i++) t.m[i] = full.m[i];
    #pragma unroll
    for (int i = 0; i < 4; i++) t.s[i] = full.s[i];
    t.n = 16;
    stats_float<RANK_CH>(rfull, t);
}

template <int FIT_CH, int RANK_CH>
__device__ __forceinline__ int32_t merge_key(const Win& w, const Tex& tx, const SeedTables& T)
{
    if (w.key >= 0) return w.key;
    Stats<RANK_CH> rfull;
    whole_block_rank_stats<FIT_CH, RANK_CH>(rfull, tx);
    return rank_key<RANK_CH>(w.shape, tx, rfull, T);
}

// ---- FUSED deep path: whole surfaces in two launches --------------------------------------------------------------------
// The kernels above run as up to seven launches, each re-reading the 64 B block from HBM and handing winners, best error
// and the current block to the next through the workspace: 5.4x the algorithmic bytes for a `slow` call.  Nothing in
// that chain needs a kernel boundary except the register budgets (scans: 4 waves per SIMD; refinement: 2).  So:
//   bc7_scan_all    ONE launch for the scans of the three-channel families {0,2} and {1,3} (mode 7, whose four-channel
//                   fits need more registers, gets its own).  Workgroup ids are mapped XCD-aware: MI355X deals consecutive
//                   workgroups round-robin to its 8 XCDs, each with its own L2, so (chunk, family) = f(workgroup id) runs
//                   256 chunks of one family, then the SAME chunks of the other, every chunk on the same XCD both times
//                   -- the second family's texel loads hit that L2 instead of HBM, while a CU still runs one family's
//                   code for long stretches.  Winners leave as 4 bytes per mode: error (< 2^23: 16 texels x 4 channels
//                   x 255^2) << 7 | shape;
//   bc7_finish_all  ONE launch: each lane refines its modes' winners in the reference's order 0,2,1,3,7, then modes
//                   4,5,6, carrying best error and block in registers, and writes the block once.
// RGBA profiles (channels == 4) with both mode groups enabled run the same kernels in the order  scan 7 -> finish<1> (modes
// 7,4,5,6; leaves block + error) -> scan {0,2},{1,3} -> finish<2> (modes 0,2,1,3; replaces the block iff its error <= the
// alpha group's, which is the reference's first-strict-minimum over 0,2,1,3,7,4,5,6).  A three-channel mode's error includes
// sum (255 - alpha)^2, so waves whose 64 blocks all have that term above their alpha-group error skip the RGB scans and
// their refinement: on translucent content most of the call (alpha_slow 10.7 -> 4.7 ms at 4096^2), on opaque content nothing
// is skipped and the result is the same bytes either way.
// HBM bytes per block: 64 (scans, shared through L2) + 64 (finish) + 2 x 4 x modes + 16 = ~176: 2.1x algorithmic.
__device__ __forceinline__ uint32_t pack_win(const Win& w) { return w.err == ERR_MAX ? 0xffffffffu : (((uint32_t)w.err << 7) | ((uint32_t)w.shape & 127u)); }
__device__ __forceinline__ void unpack_win(Win& w, uint32_t v)
{
    if (v == 0xffffffffu) { w.err = ERR_MAX; w.shape = 0; } else { w.err = (int32_t)(v >> 7); w.shape = (int32_t)(v & 127u); }
    w.key = -1;
}

#ifndef LIST_SCAN_MAX_PARTS
#define LIST_SCAN_MAX_PARTS 8
#endif
// split scans of the fused path (bounded order, modes 1/3 over a short list): how many strided shares of the 64 shapes each listed block's
// scan is cut into so that a short list still fills the chip -- a function of the list length alone, computed alike by the scan and by
// the refinement that merges the shares.  parts x listed blocks <= nblocks: the shares' winners fit the mode's winner row, [part][slot].
__device__ __forceinline__ int32_t list_scan_parts(int32_t count, int32_t nblocks)
{
    const int32_t chunks = ((count + TPB - 1) / TPB + 7) & ~7;        // in eights: a chunk's shares stay on one XCD (below)
    if (chunks <= 0) return 1;
    const int32_t p = nblocks / (chunks * TPB);
    return p < 1 ? 1 : (p > LIST_SCAN_MAX_PARTS ? LIST_SCAN_MAX_PARTS : p);
}
// ordered argmin over the shares' winners of mode 1 / 3 (packed: the rank key is evaluated on a tie only, as in the wide path)
template <int FIT_CH, int RANK_CH>
__device__ __forceinline__ void merge_packed_parts(Win& w, Lane& ln, const uint32_t* __restrict__ row, int32_t count, int parts, int32_t slot)
{
    unpack_win(w, row[slot]);
    for (int p = 1; p < parts; p++) {
        Win x;
        unpack_win(x, row[(int64_t)p * count + slot]);
        if (x.err < w.err) { w = x; continue; }
        if (x.err != w.err || x.err == ERR_MAX) continue;
        w.key = merge_key<FIT_CH, RANK_CH>(w, ln.tx, ln.T); x.key = merge_key<FIT_CH, RANK_CH>(x, ln.tx, ln.T);
        if (x.key < w.key) w = x;
    }
}

// the pair route of the RGB bounded order (PAIRS, below bc7_pilot_estimate)
// ctr, a band's counters: [0..63] bucket lengths, [64] overflow, [65] the second list's length, [66] the band's list length, [68..] its PairTarget
struct PairRegion { uint64_t* words; int32_t* buckets; int32_t* ctr; int32_t cap; };
constexpr int PAIR_CTR_OVERFLOW = 64, PAIR_CTR_REDO = 65, PAIR_CTR_LIST = 66, PAIR_CTR_TARGET = 68, PAIR_CTR_WORDS = 80;
// where bc7_finish_all<3> leaves a band's pairs (words == nullptr: the pair route is off).  It lies in device memory at a fixed distance from the
// list length the kernel is given anyway (bc7_bounded_setup writes it at the start of the call) and is read at the end of the kernel: as kernel
// arguments the nine words are loaded at the kernel's entry and held in SGPRs through the whole refinement, which answers with more spills
// (tools/kernel_resources.py)
struct PairTarget { PairRegion P; int32_t* redo; };
static_assert(sizeof(PairTarget) <= (PAIR_CTR_WORDS - PAIR_CTR_TARGET) * sizeof(int32_t) && PAIR_CTR_TARGET % 2 == 0 && PAIR_CTR_WORDS % 4 == 0, "PairTarget behind the counters");
constexpr int PAIR_MAX_PER_BLOCK = 32;
// The call's counter block (FusedLayout::counts): CTR_WORDS words that the call's setup clears, then both bands' pair counters (PAIR_CTR_WORDS each).
// A band keeps three consecutive list lengths: of the RGBA profiles' block lists (where an RGB mode, modes 1/3, mode 7 can win), or -- the RGB bounded
// order -- of its three rotation lists.  Band 1's triple is the same words in either order; a call without bands uses band 0's.
constexpr int CTR_LIST_RGB = 0, CTR_LIST_13 = 1, CTR_LIST_7 = 2;    // band 0 of the alpha-first orders (band 1: CTR_BAND1 + the same)
constexpr int CTR_ROT = 3;                                          // band 0's rotation lists [3] (band 1: CTR_BAND1)
constexpr int CTR_PILOT_FLAG = 6;                                   // the pilot's verdict
constexpr int CTR_PILOT = 8;                                        // the pilot's counters [3]:
constexpr int PILOT_LISTED = 0, PILOT_SAMPLED = 1, PILOT_DONE = 2;  //   blocks its estimate lists, blocks it looked at, workgroups done
constexpr int CTR_BAND1 = 11;                                       // band 1's three list lengths
constexpr int CTR_WORDS = 16;
static_assert(CTR_ROT + 3 <= CTR_PILOT_FLAG && CTR_PILOT + 3 <= CTR_BAND1 && CTR_BAND1 + 3 <= CTR_WORDS, "the counter words do not overlap");
// ROT TASKS (bc7_rot_tasks' header).  Per band: three rotation lists of `cap` block ids, their lengths (three consecutive words the call's
// setup clears), and a payload slot per (rotation, list position); per block of the surface one merged word
//   error << 32 | mode 5 << 31 | rotation << 29 | list position        (~0: no candidate)
// whose 64-bit minimum is the reference's first strict minimum over modes 4 then 5, rotations in order.  29 bits of position hold the
// 8.4 M blocks of a band of a 16 384^2 call (and the 16.8 M of a call without bands).
struct RotRegion { int32_t* lists; int32_t* counts; unsigned long long* words; uint4* payload; int32_t cap; };
constexpr int ROT_WORD_ROT_SHIFT = 29, ROT_WORD_MODE5_SHIFT = 31;
constexpr unsigned long long ROT_WORD_POS_MASK = (1ull << ROT_WORD_ROT_SHIFT) - 1ull;
constexpr unsigned long long PAIR_WORD_HEAVY = ~0ull - 1ull;        // no merged word takes this value: errors stay below 2^23

struct ScanTasks { int n; int kind[3]; };      // WK_SCAN02 / WK_SCAN13 / WK_SCAN7 in launch order

// Round 5, the BANDS and the PILOT of the bounded order (launch_rgb_bounded, launch_alpha_first_bounded7): which chunks (runs of TPB blocks) of the surface a launch of
// bc7_scan_all / bc7_finish_all walks, and whether it runs at all.
//   kind 0  every chunk: workgroup i -> chunk i
//   kind 2  every eighth chunk (8 i + 3): what bc7_pilot_estimate looks at, for a probe that scans nothing else
//   kind 1  a BAND: the surface is cut into stripes of `stripe` chunks, even stripes are band 0, odd stripes band 1 (two interleaved
//           halves, so that both see all of the surface's content); workgroup i takes the i-th chunk of band `band`
// `gate` (optional): a device word written by bc7_pilot_estimate before this launch starts; the launch returns at once unless it holds
// `want` -- both mode orders are enqueued behind the pilot and the device picks one, without a host round trip.
struct ChunkSel { int32_t kind, stripe, band; const int32_t* gate; int32_t want; };
__device__ __forceinline__ int32_t sel_chunk(const ChunkSel& s, int32_t i)
{
    if (s.kind == 0) return i;
    if (s.kind == 2) return i * 8 + 3;
    const int32_t q = i / s.stripe;
    return (2 * q + s.band) * s.stripe + (i - q * s.stripe);
}

// FAM7 = false: the three-channel families {0,2} and {1,3} (4 waves per SIMD; ranked lists 3); FAM7 = true: the mode 7 scan
// alone (four-channel fits need more registers; sharing a kernel with the others made those spill.  Unranked 4 waves since the
// max-ILP schedule, ranked lists 2).
__host__ __device__ constexpr int scan_all_waves(bool ranked, bool fam7) { return fam7 ? (ranked ? SWR27 : SW7) : (ranked ? SWR2 : SWALL); }
template <bool VEC16, bool RANKED_LISTS, bool FAM7>
__global__ void __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(scan_all_waves(RANKED_LISTS, FAM7), scan_all_waves(RANKED_LISTS, FAM7))))
bc7_scan_all(const uint8_t* __restrict__ src, int64_t stride, int32_t blocks_x, int32_t nblocks, uint32_t* __restrict__ wins4,
             const bc7_enc_settings S, const ScanTasks tasks, const int ranked13, const int ranked7, const int32_t nchunks, const int32_t grain,
             const int32_t* __restrict__ rgb_list, const int32_t* __restrict__ rgb_count, const int32_t split, const ChunkSel sel,
             const uint4* __restrict__ compact)
{
    __shared__ unsigned short s_seed16[2048];
    __shared__ uint32_t s_seed32[2048];
    // ranked lists: 2 subsets x 8 levels (3 waves per SIMD: 3 x 44 KiB); else 12 levels and, for search_02, its mode 0 cache (4 x 40 KiB)
    __shared__ uint2 s_pal[(RANKED_LISTS ? 16 : (FAM7 ? 12 : 14)) * TPB];
    if (sel.gate && *sel.gate != sel.want) return;                  // the pilot chose the other order (whole grid: no barrier is pending)
    if (!RANKED_LISTS && split) {
        // bounded order: modes 1/3 (or mode 7: FAM7) over the list bc7_finish_all<.., 3 | 5 | 6> left, each listed block's 64 shapes cut
        // into `parts` strided shares (list_scan_parts) so that a short list still fills the chip; winners go to [part][slot] of the modes' rows
        const int32_t count = *rgb_count;
        const int32_t parts = list_scan_parts(count, nblocks);
        // workgroup w runs on XCD w % 8: the shares of a chunk are 8 workgroups apart, so they read its texels through the same L2
        const uint32_t wg = blockIdx.x;
        const int32_t chunk = (int32_t)((wg / (8u * (uint32_t)parts)) * 8u + (wg & 7u)), part = (int32_t)((wg >> 3) % (uint32_t)parts);
        if (chunk * TPB >= count) return;                                // whole workgroup: no barrier is pending
        Lane ln;
        ln.T = stage_seed_tables_fast(s_seed16, s_seed32, threadIdx.x, TPB);
        __syncthreads();
        const int32_t gid = chunk * TPB + threadIdx.x;
        const bool live = gid < count;
        const int32_t slot = live ? gid : count - 1;
        ln.keys = nullptr;
        ln.pal = s_pal + threadIdx.x;
        if (compact) load_block_compact(ln.tx, compact, slot); else load_block<VEC16>(ln.tx, src, stride, blocks_x, rgb_list[slot]);
        Win wa, wb;
        if (FAM7) {
            search_two_subset<true, 4, 0>(ln, S, wa, wb, part, parts);             // RGBA profiles only (launch_bc7)
            if (live) wins4[(int64_t)wide_win_slot(7) * nblocks + (int64_t)part * count + slot] = pack_win(wa);
        } else {
            search_two_subset<false, 3, 0>(ln, S, wa, wb, part, parts);
            if (live) {
                wins4[(int64_t)wide_win_slot(1) * nblocks + (int64_t)part * count + slot] = pack_win(wa);
                wins4[(int64_t)wide_win_slot(3) * nblocks + (int64_t)part * count + slot] = pack_win(wb);
            }
        }
        return;
    }
    // `grain` chunks of one family, then the same chunks of the next family (grain is a multiple of 8, so a chunk's
    // families run on the same XCD: workgroup w -> XCD w % 8)
    const uint32_t w = blockIdx.x, per = (uint32_t)grain * (uint32_t)tasks.n, group = w / per, r = w % per;
    const int t = (int)(r / (uint32_t)grain);
    const int32_t chunk_i = (int32_t)(group * (uint32_t)grain + r % (uint32_t)grain);
    if (chunk_i >= nchunks) return;                                  // whole workgroup: no barrier is pending
    const int32_t chunk = sel_chunk(sel, chunk_i);                   // nchunks counts the chunks `sel` selects
    // RGBA profile, alpha-capable modes already encoded (bc7_finish_all<.., 1>): an RGB-only mode's error includes
    // sum (alpha - 255)^2 (kernel.ispc:1267-1277, 1356), so where that term alone exceeds the alpha modes' best error no
    // three-channel mode can win or tie.  Round 3: finish<1> COMPACTS the blocks where an RGB mode can still win or tie into
    // rgb_list (any order: blocks are independent), and this kernel walks the list instead of the surface -- lanes are
    // filled with blocks that need the scans whatever their position, so a surface whose opaque and translucent blocks are
    // mixed at random pays for the opaque half only (round 2 skipped whole waves: nothing on such content).
    const int32_t nact = (!FAM7 && rgb_list) ? *rgb_count : nblocks;
    if (chunk * TPB >= nact) return;
    Lane ln;
    ln.T = stage_seed_tables_fast(s_seed16, s_seed32, threadIdx.x, TPB);
    __syncthreads();
    const int32_t gid = chunk * TPB + threadIdx.x;
    const bool live = gid < nact;
    const int32_t slot = live ? gid : nact - 1;                      // idle lanes of the last workgroup redo its last block, store nothing
    const int32_t b = (!FAM7 && rgb_list) ? rgb_list[slot] : slot;
    ln.keys = nullptr;
    ln.pal = s_pal + threadIdx.x;
    load_block<VEC16>(ln.tx, src, stride, blocks_x, b);
    const int kind = tasks.kind[t];                                  // wave-uniform
    Win wa, wb;
    if (!FAM7 && kind == WK_SCAN02) {
        search_02<true>(ln, S, wa, wb);
        if (live) { wins4[(int64_t)wide_win_slot(0) * nblocks + b] = pack_win(wa); if (!S.skip_mode2) wins4[(int64_t)wide_win_slot(2) * nblocks + b] = pack_win(wb); }
    } else if (!FAM7) {
        if (RANKED_LISTS && ranked13) search_two_subset<false, 3, 2>(ln, S, wa, wb); else search_two_subset<false, 3, 0>(ln, S, wa, wb);
        if (live) { wins4[(int64_t)wide_win_slot(1) * nblocks + b] = pack_win(wa); wins4[(int64_t)wide_win_slot(3) * nblocks + b] = pack_win(wb); }
    } else {
        if (S.channels == 4) { if (RANKED_LISTS && ranked7) search_two_subset<true, 4, 2>(ln, S, wa, wb); else search_two_subset<true, 4, 0>(ln, S, wa, wb); }
        else                 { if (RANKED_LISTS && ranked7) search_two_subset<true, 3, 2>(ln, S, wa, wb); else search_two_subset<true, 3, 0>(ln, S, wa, wb); }
        if (live) wins4[(int64_t)wide_win_slot(7) * nblocks + b] = pack_win(wa);
    }
}

// appends block `b` of the lanes with `need` to a list: one atomic per wave, ranks within the wave by ballot (any order: blocks are independent)
// returns the block's position in the list (-1: not appended)
__device__ __forceinline__ int32_t append_to_list(int32_t* __restrict__ list, int32_t* __restrict__ count, bool need, int32_t b)
{
    const unsigned long long m = __ballot(need);
    int32_t pos = -1;
    if (m) {
        const int lane = (int)(threadIdx.x & 63u);
        int32_t base = 0;
        if (lane == 0) base = atomicAdd(count, (int32_t)__popcll(m));
        base = __shfl(base, 0);
        if (need) { pos = base + (int32_t)__popcll(m & ((1ull << lane) - 1ull)); list[pos] = b; }
    }
    return pos;
}
// the same for the three rotation lists of a band at once, claimed per WORKGROUP: every wave leaves its three popcounts in `s_cnt`, three lanes
// of the workgroup add the totals to the three consecutive list lengths in one atomic instruction and turn the popcounts into each wave's
// base, and the lanes write behind it.  Two barriers and one atomic instruction per workgroup where the per-wave append made twelve atomics, each
// waited for by its whole wave (the lengths share a cache line that every XCD contends for).  Every thread of the workgroup has to get here, idle
// lanes included.  `s_cnt` is storage of its own: other waves of the workgroup may still be refining out of s_pal when the first one arrives.
__device__ __forceinline__ void append_to_rotation_lists(int32_t (*s_cnt)[4], const RotRegion& R, bool need0, bool need1, bool need2, int32_t b)
{
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned long long m0 = __ballot(need0), m1 = __ballot(need1), m2 = __ballot(need2);
    if (lane < 3) s_cnt[wave][lane] = (int32_t)__popcll(lane == 0 ? m0 : (lane == 1 ? m1 : m2));
    __syncthreads();
    if (threadIdx.x < 3u) {
        int32_t t = 0;
#pragma unroll
        for (int w = 0; w < TPB / 64; w++) t += s_cnt[w][lane];
        int32_t base = t ? atomicAdd(R.counts + lane, t) : 0;        // nothing to claim (modes 4/5 off, no survivor): no atomic
#pragma unroll
        for (int w = 0; w < TPB / 64; w++) { const int32_t c = s_cnt[w][lane]; s_cnt[w][lane] = base; base += c; }
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    if (need0) R.lists[                      s_cnt[wave][0] + (int32_t)__popcll(m0 & below)] = b;
    if (need1) R.lists[(int64_t)R.cap     + s_cnt[wave][1] + (int32_t)__popcll(m1 & below)] = b;
    if (need2) R.lists[(int64_t)R.cap * 2 + s_cnt[wave][2] + (int32_t)__popcll(m2 & below)] = b;
}

// PHASE 0: every mode, reference order (RGB profiles).  RGBA profiles run in two phases so that the three-channel modes can be
// skipped where they cannot win: PHASE 1 = the alpha-capable modes 7,4,5,6 (their relative order kept), leaves the block and
// its error; PHASE 2 = modes 0,2,1,3 for the waves that still need them, then the reference's choice between the two groups:
// the first strict minimum over 0,2,1,3,7,4,5,6 is the RGB group's winner iff its error <= the alpha group's.
//
// Round 4, the BOUNDED order (profiles that scan every two-subset shape: `slow`, `alpha_slow`): modes 1 and 3 run LAST, and only for the
// blocks where some two-subset shape's exact lower bound (two_subset_bound, bc7_exact.hpp) is still below what the other modes achieved.
//   PHASE 3 (RGB profiles)   modes 0,2 then 4,5,6 -> block, and the incumbent `inc` modes 1/3 have to get strictly below: the error,
//                            + 1 when it belongs to mode 4/5/6 (those come after 1/3 in the reference's order, so a tie goes to 1/3);
//                            then the list of blocks with min over shapes of the bound < inc;
//   PHASE 5 (RGBA profiles)  the same on the list PHASE 1 left: modes 0,2, the choice against the alpha group (ties to 0/2), inc, list;
//   PHASE 4                  modes 1,3 over that list, starting from best_err = inc: the block is replaced iff one of them gets below.
// RGBA profiles whose mode 7 scans every shape too (`alpha_slow`) bound it with the same number (a mode 7 encoding's colour part is one more
// set of rounded points of a segment per subset; its error has no opaque term):
//   PHASE 6                  modes 4,5,6 alone -> block, error; the list of blocks where a three-channel mode can still win or tie, as
//                            PHASE 1 leaves it (judged against modes 4,5,6 only: a longer list, the same final comparison), and for the
//                            other blocks inc = error + 1 and a place on mode 7's list (translucent content: not bounded, mode 7 is its mode);
//   PHASE 5                  as above, and it also appends the blocks whose mode 7 bound is below inc to mode 7's list;
//   PHASE 4                  as above, and leaves inc = its error where it replaced the block (mode 7 comes after 1/3: strictly below);
//   PHASE 7                  mode 7 over its list from best_err = inc.
// The final block is the reference's first strict minimum over 0,2,1,3,7,4,5,6 either way: a mode's result enters only through
// `err < best_err`, the groups keep their internal order, and a skipped block's modes 1/3 cannot reach inc whatever shape their scan would
// have picked (every encoding of every shape is bounded).
// Round 5: mode 6 under an RGB profile (kernel.ispc:1657-1689, channels == 3) decodes every texel to a ROUNDED point of ONE segment in RGB,
// so its error is >= (sqrt(R) - sqrt(3)/2 sqrt(16))_+^2 with R the block's residual about its best line (subset_residual_bound: the same
// number the two-subset bound is built from, for the whole block), and it replaces the block only on a strict `<`.  Where that bound has
// already been reached by the modes before it for all 64 blocks of the wave, mode 6 is not run (per-lane skipping saves nothing on a SIMT
// machine).  profiles/history/r05/r05_bc7_bound456_study.txt: 100 % of the bench surface's blocks (noise in every block: three subsets beat one line),
// 56-64 % of a photograph's; modes 4/5 cannot be bounded out this way (15 % / 1 %: their scalar channel absorbs the noise).
__device__ __forceinline__ bool mode6_cannot_win(Lane& ln)
{
    if (__all(ln.best_err == 0)) return true;
    IStats<3> full;
    stats_int<3>(full, ln.tx.pl, whole_block());
    const float d = __builtin_amdgcn_sqrtf(subset_residual_bound(full) * rcp_of_count(16)) * 0.999999f - BOUND_SLACK3[16];
    const float e = fmaxf(d, 0.0f);
    const float lb = e * e * 0.999999f;
    return __all(lb >= (float)ln.best_err);                        // errors are integers below 2^24: exact as floats
}

#ifndef FINISH_ALL_WAVES
#define FINISH_ALL_WAVES 2
#endif
#ifndef BOUND_BAIL_AFTER
#define BOUND_BAIL_AFTER 4
#endif
#ifndef BOUND_BAIL_LANES
#define BOUND_BAIL_LANES 40
#endif
// The TAIL of the bounded orders' first refinement (PHASE 3 and PHASE 5 call it in place; bc7_bound_list, below bc7_finish_all, is PHASE 10's): the
// one copy of the rules by which a block whose incumbent is `inc` (already in inc_err) gets on the list of modes 1/3 -- the 64 two-subset bounds,
// the per-wave append or the workgroup's claim, the pairs bucketed by shape, the heavy blocks to the second list, the compact texels -- and,
// PHASE 5 only (`out_list7`), on mode 7's list.  TAIL3: the RGB order, whose `out_count` has the band's PairTarget behind it.  `s_at` ([TPB / 64][64]
// under TAIL3) and `s_listed` are the workgroup's LDS for the claim; every lane of the workgroup calls, idle lanes (`live` false) too: the claim
// holds two barriers.
template <bool TAIL3, int AT_ROWS>
__device__ __forceinline__ void bounded_list_tail(Tex& tx, const int32_t inc, const int32_t opaque_err, const bool live, const int32_t b,
                                                  int32_t (&s_at)[AT_ROWS][64], int32_t (&s_listed)[TPB / 64], int32_t* __restrict__ out_list, int32_t* __restrict__ out_count,
                                                  int32_t* __restrict__ out_list7, int32_t* __restrict__ out_count7, uint4* __restrict__ out_compact)
{
    tx.fence();
    IStats<3> full;
    stats_int<3>(full, tx.pl, whole_block());
    const float lim = (float)(inc - opaque_err) - 0.5f;            // errors are integers: a bound above inc - 1 already rules the shape out
    const float lim7 = (float)inc - 0.5f;                           // mode 7 carries no opaque term
    const bool with7 = !TAIL3 && out_list7 != nullptr;              // wave-uniform
    // PAIRS (header above bc7_pair_scan): this launch also leaves the (block, shape) pairs of the listed blocks, so every shape is
    // bounded for every lane -- no early exit, no bail -- and the lane keeps a bit per shape instead of `need` alone
    // CONTRACT of TAIL3: `out_count` is word PAIR_CTR_LIST of a band's counter block that bc7_bounded_setup has filled in this call, so the
    // band's PairTarget lies PAIR_CTR_TARGET - PAIR_CTR_LIST words behind it (the launcher refuses any other pointer)
    const PairTarget* target = nullptr;
    if (TAIL3) target = reinterpret_cast<const PairTarget*>(out_count + (PAIR_CTR_TARGET - PAIR_CTR_LIST));
    const bool pairs = TAIL3 && target->P.words != nullptr;         // grid-uniform
    bool need = !live, need7 = !live || !with7;                     // idle lanes never hold the loop up
    unsigned long long mine = 0, any = 0;                           // shapes whose bound is below `lim`: the lane's, the wave's (scalar)
#pragma unroll 1
    for (int shape = 0; shape < 64; shape++) {
        if (!pairs) {
            if (__all(need && need7)) break;
            // a wave most of whose blocks need the modes anyway stops bounding the others (visiting a block is always allowed):
            // content the bound does not separate pays for a few shapes, not for 64
            if (shape == BOUND_BAIL_AFTER && __popcll(__ballot(need && need7)) >= BOUND_BAIL_LANES) { need = true; need7 = true; break; }
        }
        const float lb = two_subset_bound(shape, tx.pl, full);
        const bool in = !(lb >= lim);
        need = need || in;
        need7 = need7 || !(lb >= lim7);
        if (pairs) {
            mine |= (live && in) ? (1ull << shape) : 0ull;
            any |= __ballot(live && in) ? (1ull << shape) : 0ull;
        }
    }
    int32_t pos = -1;                                               // the block's position in the list: its slot
    if (!pairs) pos = append_to_list(out_list, out_count, live && need, b);
    else {
        // `pos` is the block's slot: its merged words, its compact texels, what the buckets hold.  The list's stretch is claimed per
        // WORKGROUP together with the buckets' -- the list length is the 65th counter of that claim, no atomic per wave that the whole wave
        // waits for before it can write anything -- so everything that needs `pos` follows the claim.  A block more than half of whose
        // shapes survive (photograph-like content inside a surface the pilot gave the bounded order) is cheaper in the full list scan,
        // which takes the 64 shapes without rank keys: straight to the second list, no pairs, its words say so
        // (lane and wave formed here, not from an expression of threadIdx the kernel's head also has: that one would be kept -- spilled --
        // through the refinement)
        const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const PairRegion P = target->P;
        const bool heavy = __popcll(mine) > PAIR_MAX_PER_BLOCK;
        if (heavy) mine = 0;
        const unsigned long long listed = __ballot(live && need);
        // survivors per (wave, shape): lane s carries shape s's count (shapes nobody in the wave keeps are not visited).  No global
        // atomic per (wave, shape): each one waited for, that made the first builder latency bound (1.0 ms instead of 0.1)
        int32_t k = 0;
        for (unsigned long long rest = any; rest; rest &= rest - 1ull) {
            const int shape = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(rest));
            const int32_t c = (int32_t)__popcll(__ballot((mine >> shape) & 1ull));
            k = (lane == shape) ? c : k;
        }
        s_at[wave][lane] = k;
        if (lane == 0) s_listed[wave] = (int32_t)__popcll(listed);
        __syncthreads();
        if (threadIdx.x < 64u) {                                    // the workgroup's stretch of each bucket: 64 atomics, one instruction
            int32_t t = 0;
#pragma unroll
            for (int w = 0; w < TPB / 64; w++) t += s_at[w][lane];
            int32_t base = t ? atomicAdd(P.ctr + lane, t) : 0;
            if (base + t > P.cap) { P.ctr[PAIR_CTR_OVERFLOW] = 1; base = -1; }
#pragma unroll
            for (int w = 0; w < TPB / 64; w++) { const int32_t c = s_at[w][lane]; s_at[w][lane] = base; base = base < 0 ? -1 : base + c; }
        } else if (threadIdx.x == 64u) {                            // and its stretch of the list: the first wave's 64 lanes are taken, so the
            int32_t t = 0;                                          // second wave issues this one beside them
#pragma unroll
            for (int w = 0; w < TPB / 64; w++) t += s_listed[w];
            int32_t base = t ? atomicAdd(out_count, t) : 0;
#pragma unroll
            for (int w = 0; w < TPB / 64; w++) { const int32_t c = s_listed[w]; s_listed[w] = base; base += c; }
        }
        __syncthreads();
        if (live && need) { pos = s_listed[wave] + (int32_t)__popcll(listed & ((1ull << lane) - 1ull)); out_list[pos] = b; }
        if (pos >= 0) { P.words[2 * (int64_t)pos] = heavy ? PAIR_WORD_HEAVY : ~0ull; P.words[2 * (int64_t)pos + 1] = ~0ull; }
        append_to_list(target->redo, P.ctr + PAIR_CTR_REDO, heavy, b);
        const int32_t at = s_at[wave][lane];                        // lane s: where the wave's survivors of shape s go
        for (unsigned long long rest = any; rest; rest &= rest - 1ull) {
            const int shape = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(rest));
            const bool in = (mine >> shape) & 1ull;
            const unsigned long long m = __ballot(in);
            const int32_t base = __builtin_amdgcn_readlane(at, shape);
            if (in && base >= 0) P.buckets[(int64_t)shape * P.cap + base + (int32_t)__popcll(m & ((1ull << lane) - 1ull))] = pos;
        }
    }
    if (out_compact && pos >= 0) {                                  // the listed block's texels, in list order (load_block_compact)
        uint4* c = out_compact + (int64_t)pos * 4;
#pragma unroll
        for (int y = 0; y < 4; y++) c[y] = make_uint4(tx.w[y * 4 + 0], tx.w[y * 4 + 1], tx.w[y * 4 + 2], tx.w[y * 4 + 3]);
    }
    if (with7) append_to_list(out_list7, out_count7, live && need7, b);
}

// PHASE 10 holds three workgroups per CU (mode 6's 16-level palette leaves 44 KiB of LDS); the refinement phases two (214-256 VGPRs)
#ifndef FINISH10_WAVES
#define FINISH10_WAVES 3
#endif
#ifndef FINISH10_PAL_LEVELS
#define FINISH10_PAL_LEVELS 16
#endif
__host__ __device__ constexpr int finish_all_waves(int phase) { return phase == 10 ? FINISH10_WAVES : FINISH_ALL_WAVES; }
template <bool VEC16, int PHASE>
__global__ void __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(finish_all_waves(PHASE), finish_all_waves(PHASE))))
bc7_finish_all(const uint8_t* __restrict__ src, int64_t stride, int32_t blocks_x, int32_t nblocks, uint8_t* __restrict__ dst,
               const uint32_t* __restrict__ wins4, const bc7_enc_settings S, int32_t* __restrict__ inc_err,
               const int32_t* __restrict__ in_list, const int32_t* __restrict__ in_count, int32_t* __restrict__ out_list, int32_t* __restrict__ out_count,
               int32_t* __restrict__ out_list7, int32_t* __restrict__ out_count7, const ChunkSel sel,
               const uint4* __restrict__ in_compact, uint4* __restrict__ out_compact, const RotRegion R)
{
    constexpr bool LISTED = PHASE == 2 || PHASE == 4 || PHASE == 5 || PHASE == 7 || PHASE == 8;   // walks a compacted list of an earlier phase
    constexpr bool DO02 = PHASE == 0 || PHASE == 2 || PHASE == 3 || PHASE == 5 || PHASE == 9;
    constexpr bool TAIL3 = PHASE == 3 || PHASE == 10;                // leaves the incumbent, the list and the pairs of the RGB bounded order
    constexpr bool DO13 = PHASE == 0 || PHASE == 2 || PHASE == 4;
    constexpr bool DO7 = PHASE == 0 || PHASE == 1;
    constexpr bool DO456 = PHASE == 0 || PHASE == 1 || PHASE == 3 || PHASE == 6;
    __shared__ unsigned short s_seed16[2048];
    __shared__ uint32_t s_seed32[2048];
    __shared__ uint2 s_pal[(PHASE == 10 ? FINISH10_PAL_LEVELS : LANE_PAL_LEVELS) * TPB];   // refinement: a palette per subset of the lane's winner (PHASE 10: mode 6's 16 levels)
    __shared__ int32_t s_at[PHASE == 3 ? TPB / 64 : 1][64];           // PAIRS: per (wave, shape) the survivors, then where they go in the bucket (its own
                                                                    // kilobyte: other waves of the workgroup still use s_pal when the first one gets here)
    __shared__ int32_t s_listed[TPB / 64];                           // PAIRS: per wave the blocks it lists, then its base in the list (the 65th counter)
    __shared__ int32_t s_rot[PHASE == 9 ? TPB / 64 : 1][4];       // PHASE 9: per (wave, rotation) the listed blocks, then the wave's base in the list
    if (sel.gate && *sel.gate != sel.want) return;                   // the pilot chose the other order (whole grid: no barrier is pending)
    const int32_t nact = LISTED ? *in_count : nblocks;
    const int32_t chunk = LISTED ? (int32_t)blockIdx.x : sel_chunk(sel, (int32_t)blockIdx.x);
    if (chunk * TPB >= nact) return;                                 // whole workgroup, before any barrier (a band's grid is whole stripes)
    Lane ln;
    ln.T = stage_seed_tables_fast(s_seed16, s_seed32, threadIdx.x, TPB);
    __syncthreads();
    const int32_t gid = chunk * TPB + threadIdx.x;
    const bool live = gid < nact;
    const int32_t slot = live ? gid : nact - 1;
    const int32_t b = LISTED ? in_list[slot] : slot;
    ln.keys = nullptr;
    ln.pal = s_pal + threadIdx.x;
    if (LISTED && in_compact) load_block_compact(ln.tx, in_compact, slot); else load_block<VEC16>(ln.tx, src, stride, blocks_x, b);
    ln.best_err = ERR_MAX;
    ln.best[0] = ln.best[1] = ln.best[2] = ln.best[3] = 0u;
    ln.improved = false;
    ln.opaque_err = 0;                                                             // kernel.ispc:1267-1277
    if (S.channels == 4) {
        uint32_t e = 0;
#pragma unroll
        for (int d = 0; d < 4; d++) { const uint32_t x = ~ln.tx.pl[3][d]; e = udot4(x, x, e); }
        ln.opaque_err = (int32_t)e;
    }
    const bool on13 = S.mode_selection[1];
    int32_t e_alpha = ERR_MAX;
    if (PHASE == 2 || PHASE == 5) e_alpha = inc_err[b];      // every listed block has opaque_err <= e_alpha: its winners exist
    if (PHASE == 4 || PHASE == 7 || PHASE == 8 || PHASE == 10) ln.best_err = inc_err[b];  // what modes 1/3 (mode 7; PHASE 10: modes 4,5,6) have to get strictly below
    Win w;
    if (DO02 && S.mode_selection[0]) {
        unpack_win(w, wins4[(int64_t)wide_win_slot(0) * nblocks + b]);
        refine_and_commit<0>(ln, w, S.refineIterations[0], S.channels);
        if (!S.skip_mode2) { ln.tx.fence(); unpack_win(w, wins4[(int64_t)wide_win_slot(2) * nblocks + b]); refine_and_commit<2>(ln, w, S.refineIterations[2], S.channels); }
    }
    const int32_t e02 = ln.best_err;
    if (PHASE == 9) {
        // ROT TASKS (bc7_rot_tasks' header): the block as modes 0/2 leave it is stored below; e02 is what modes 4,5,6 have to get strictly
        // below; the block's merged word starts empty; and the block goes on the list of every rotation whose exact bound (rotation_bound,
        // bc7_exact.hpp) is still below e02 - 1/2 (errors are integers, modes 4/5 replace the block only on a strict `<`)
        if (live) { inc_err[b] = e02; R.words[b] = ~0ull; }
        ln.tx.fence();
        IStats<3> full;
        stats_int<3>(full, ln.tx.pl, whole_block());
        const float lim = (float)e02 - 0.5f;
        const bool on45 = live && S.mode_selection[2];
        bool need[3];
#pragma unroll
        for (int r = 0; r < 3; r++) need[r] = on45 && r >= S.mode45_channel0 && !(rotation_bound(r, full) >= lim);
        append_to_rotation_lists(s_rot, R, need[0], need[1], need[2], b);      // idle lanes arrive too: it holds barriers
    }
    if (PHASE == 10) {
        // the one candidate bc7_rot_tasks left for the block, if any: admitted with the reference's strict `<`, then mode 6 in its place
        const unsigned long long v = R.words[b];
        const int32_t e = (int32_t)(v >> 32);
        if (v != ~0ull && e < ln.best_err) {
            const uint4 p = R.payload[(int64_t)((v >> ROT_WORD_ROT_SHIFT) & 3ull) * R.cap + (int64_t)(v & ROT_WORD_POS_MASK)];
            ln.best_err = e; ln.improved = true;
            ln.best[0] = p.x; ln.best[1] = p.y; ln.best[2] = p.z; ln.best[3] = p.w;
        }
        ln.tx.fence();
        if (S.mode_selection[3] && !mode6_cannot_win(ln)) mode_6<3>(ln, S);
    }
    if (DO13 && PHASE != 4) {
        if (on13 && S.fastSkipTreshold_mode1 > 0) { ln.tx.fence(); unpack_win(w, wins4[(int64_t)wide_win_slot(1) * nblocks + b]); refine_and_commit<1>(ln, w, S.refineIterations[1], S.channels); }
        if (on13 && S.fastSkipTreshold_mode3 > 0) { ln.tx.fence(); unpack_win(w, wins4[(int64_t)wide_win_slot(3) * nblocks + b]); refine_and_commit<3>(ln, w, S.refineIterations[3], S.channels); }
    }
    if (PHASE == 4) {                                        // the list scan left [part][slot] winners (bc7_scan_all, split)
        const int parts = list_scan_parts(nact, nblocks);
        if (S.fastSkipTreshold_mode1 > 0) { ln.tx.fence(); merge_packed_parts<3, 3>(w, ln, wins4 + (int64_t)wide_win_slot(1) * nblocks, nact, parts, slot); refine_and_commit<1>(ln, w, S.refineIterations[1], S.channels); }
        if (S.fastSkipTreshold_mode3 > 0) { ln.tx.fence(); merge_packed_parts<3, 3>(w, ln, wins4 + (int64_t)wide_win_slot(3) * nblocks, nact, parts, slot); refine_and_commit<3>(ln, w, S.refineIterations[3], S.channels); }
    }
    bool redo = false;
    if (PHASE == 8) {
        // PAIRS (bc7_pair_scan's header): `wins4` is the band's merged words, two per listed block -- the ordered argmin (fast error << 32 |
        // rank key) over the shapes the bound leaves, ~0 where it leaves none -- and `out_count7` its overflow word
        const unsigned long long* pw = reinterpret_cast<const unsigned long long*>(wins4) + 2 * (int64_t)slot;
        const int32_t inc = ln.best_err;
        const bool heavy = pw[0] == PAIR_WORD_HEAVY;          // bc7_finish_all<3> already put the block on the second list
        redo = !heavy && *out_count7 != 0;                   // a bucket overflowed: the whole band takes the full list scan
        const bool use = !heavy && !redo;
        const unsigned long long v1 = (use && S.fastSkipTreshold_mode1 > 0) ? pw[0] : ~0ull, v3 = (use && S.fastSkipTreshold_mode3 > 0) ? pw[1] : ~0ull;
        if (v1 != ~0ull) {
            ln.tx.fence();
            w.err = (int32_t)(v1 >> 32); w.key = (int32_t)(uint32_t)v1; w.shape = w.key & 63;
            const bool open = w.err + ln.opaque_err >= inc;  // a shape the bound excluded may come before this one in the reference's order
            const int32_t before = ln.best_err;
            refine_and_commit<1>(ln, w, S.refineIterations[1], S.channels);
            redo = redo || (open && ln.best_err < before);
        }
        if (v3 != ~0ull) {
            ln.tx.fence();
            w.err = (int32_t)(v3 >> 32); w.key = (int32_t)(uint32_t)v3; w.shape = w.key & 63;
            const bool open = w.err + ln.opaque_err >= inc;
            const int32_t before = ln.best_err;
            refine_and_commit<3>(ln, w, S.refineIterations[3], S.channels);
            redo = redo || (open && ln.best_err < before);
        }
        // deferred blocks keep their block and incumbent: the full list scan and bc7_finish_all<4> redo both modes for them
        append_to_list(out_list, out_count, live && redo, b);
    }
    if (PHASE == 7) {                                        // the list scan left [part][slot] winners
        const int parts = list_scan_parts(nact, nblocks);
        ln.tx.fence();
        merge_packed_parts<4, 4>(w, ln, wins4 + (int64_t)wide_win_slot(7) * nblocks, nact, parts, slot);
        refine_and_commit<7>(ln, w, S.refineIterations[7], S.channels);
    }
    if (DO7 && on13 && S.fastSkipTreshold_mode7 > 0) { ln.tx.fence(); unpack_win(w, wins4[(int64_t)wide_win_slot(7) * nblocks + b]); refine_and_commit<7>(ln, w, S.refineIterations[7], S.channels); }
    if (DO456) {
        ln.tx.fence();
        if (S.mode_selection[2]) modes_45(ln, S);
        if (S.mode_selection[3]) {
            if (S.channels == 4) mode_6<4>(ln, S);
            else if (!mode6_cannot_win(ln)) mode_6<3>(ln, S);
        }
    }
    if (PHASE == 1) {
        if (live) inc_err[b] = ln.best_err;
        // the blocks where a three-channel mode can still win or tie (its error carries sum (255 - a)^2): appended to the list the
        // RGB scans and finish<2> walk -- one atomic per wave, ranks within the wave by ballot
        append_to_list(out_list, out_count, live && ln.opaque_err <= ln.best_err, b);
    }
    if (PHASE == 6) {
        const bool rgb = ln.opaque_err <= ln.best_err;               // a three-channel mode can still win or tie (PHASE 1's rule)
        if (live) inc_err[b] = rgb ? ln.best_err : ln.best_err + 1; // PHASE 5 reads the error; PHASE 7 reads what mode 7 has to get below
        append_to_list(out_list, out_count, live && rgb, b);
        append_to_list(out_list7, out_count7, live && !rgb, b);
    }
    if (TAIL3 || PHASE == 5) {
        // incumbent of modes 1/3 (see the header), then the blocks whose modes 1/3 can still get below it
        int32_t inc;
        if (TAIL3) inc = ln.best_err + (ln.best_err < e02 ? 1 : 0);
        else            inc = (e02 <= e_alpha) ? e02 : e_alpha + 1;
        if (live) inc_err[b] = inc;
        // PHASE 10 stops here: bc7_bound_list, the next launch on the band's stream, reads `inc` back and runs the tail at its own occupancy
        if (PHASE != 10) bounded_list_tail<PHASE == 3>(ln.tx, inc, ln.opaque_err, live, b, s_at, s_listed, out_list, out_count, out_list7, out_count7, out_compact);
    }
    bool store = live;
    if (PHASE == 2 || PHASE == 5) store = store && ln.best_err <= e_alpha;   // else the alpha group's block stands (ties go to the earlier, RGB, group)
    if (PHASE == 4 || PHASE == 7 || PHASE == 10) store = store && ln.improved;   // (PHASE 10: PHASE 9 stored the block modes 0/2 left)
    if (PHASE == 8) store = store && ln.improved && !redo;
    if ((PHASE == 4 || PHASE == 8) && store) inc_err[b] = ln.best_err;         // mode 7 (PHASE 7, RGBA profiles) comes after modes 1/3: strictly below them
    if (store) {
        uint32_t* d = reinterpret_cast<uint32_t*>(dst + (int64_t)b * 16);
        if (VEC16) *reinterpret_cast<uint4*>(d) = make_uint4(ln.best[0], ln.best[1], ln.best[2], ln.best[3]);
        else { d[0] = ln.best[0]; d[1] = ln.best[1]; d[2] = ln.best[2]; d[3] = ln.best[3]; }
    }
}

// Round 11, the tail of the rotation-task order in a kernel of its own.  Behind bc7_finish_all<10> (which leaves inc in inc_err) the 64 bounds are a
// dependent chain of integer multiplies, one reciprocal and six square roots per shape that uses no LDS and needs a third of a refinement kernel's
// registers; inside PHASE 10 it ran at the two waves per SIMD the palette's LDS allows.  Here it has the claim's 1 KiB of LDS and the registers
// of BOUND_LIST_WAVES waves: 76 VGPRs, nothing spilled, six waves per SIMD (the same code at 4; at 8 two VGPRs spill and nothing is gained:
// profiles/r11_bc7_insts_valu.txt).  One chunk of the band per workgroup through the same ChunkSel, gate included; the same contract on
// `out_count` as bounded_list_tail<true>.  4096^2 bench surface 3.996 -> 3.912 ms (profiles/r11_bc7_bound_kernel_ab.txt).
#ifndef BOUND_LIST_WAVES
#define BOUND_LIST_WAVES 6
#endif
template <bool VEC16>
__global__ void __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(BOUND_LIST_WAVES, BOUND_LIST_WAVES)))
bc7_bound_list(const uint8_t* __restrict__ src, int64_t stride, int32_t blocks_x, int32_t nblocks, const int32_t channels, const int32_t* __restrict__ inc_err,
               int32_t* __restrict__ out_list, int32_t* __restrict__ out_count, const ChunkSel sel, uint4* __restrict__ out_compact)
{
    __shared__ int32_t s_at[TPB / 64][64];
    __shared__ int32_t s_listed[TPB / 64];
    if (sel.gate && *sel.gate != sel.want) return;                   // the pilot chose the other order (whole grid: no barrier is pending)
    const int32_t chunk = sel_chunk(sel, (int32_t)blockIdx.x);
    if (chunk * TPB >= nblocks) return;                              // whole workgroup, before any barrier (a band's grid is whole stripes)
    const int32_t gid = chunk * TPB + threadIdx.x;
    const bool live = gid < nblocks;                                 // idle lanes of a ragged last workgroup go on: the tail's claim holds barriers
    const int32_t b = live ? gid : nblocks - 1;
    Tex tx;
    load_block<VEC16>(tx, src, stride, blocks_x, b);
    int32_t opaque_err = 0;                                          // kernel.ispc:1267-1277
    if (channels == 4) {
        uint32_t e = 0;
#pragma unroll
        for (int d = 0; d < 4; d++) { const uint32_t x = ~tx.pl[3][d]; e = udot4(x, x, e); }
        opaque_err = (int32_t)e;
    }
    bounded_list_tail<true>(tx, inc_err[b], opaque_err, live, b, s_at, s_listed, out_list, out_count, nullptr, nullptr, out_compact);
}

// The PILOT of the bounded order (round 5).  Runs behind band 0's {0,2} scan on every eighth chunk of that band (1/16 of the surface, spread
// over it by the bands' stripes): with the scan's winners as the incumbent -- before refinement and before modes 4,5,6, so the true
// incumbent is lower and the true list shorter: an ESTIMATE from above (bench surface: 50 % estimated, 30 % listed; a photograph: 98 % and
// 94 %) -- it counts the blocks some two-subset shape's bound can still get under, with bc7_finish_all<3>'s rules, and the workgroup
// that finishes last turns the two counts into the device word the
// gated launches read: 1 = few enough blocks will need modes 1/3, the bounded order pays; 0 = nearly all will, the reference's order (one
// scan of the family over the band, one refinement kernel) is cheaper.  Nothing it computes reaches the output.
template <bool VEC16>
__global__ void __launch_bounds__(TPB)
bc7_pilot_estimate(const uint8_t* __restrict__ src, int64_t stride, int32_t blocks_x, int32_t nblocks, const uint32_t* __restrict__ wins4,
                   const int skip_mode2, const ChunkSel sel, int32_t* __restrict__ counters /* listed, sampled, done */, const int32_t thr256,
                   int32_t* __restrict__ flag, int32_t* __restrict__ host_counts /* optional: pinned host memory, {listed, sampled} for the host */)
{
    const int32_t chunk = sel_chunk(sel, (int32_t)blockIdx.x * 8 + 3);
    if (chunk * TPB < nblocks) {                                     // workgroup-uniform
        const int32_t gid = chunk * TPB + threadIdx.x;
        const bool live = gid < nblocks;
        const int32_t b = live ? gid : nblocks - 1;
        Tex tx;
        load_block<VEC16>(tx, src, stride, blocks_x, b);
        Win w0, w2;
        unpack_win(w0, wins4[(int64_t)wide_win_slot(0) * nblocks + b]);
        unpack_win(w2, skip_mode2 ? 0xffffffffu : wins4[(int64_t)wide_win_slot(2) * nblocks + b]);
        const int32_t e = min(w0.err, w2.err);
        IStats<3> full;
        stats_int<3>(full, tx.pl, whole_block());
        const float lim = (float)e - 0.5f;
        bool need = !live;
#pragma unroll 1
        for (int shape = 0; shape < 64; shape++) {
            if (__all(need)) break;
            if (shape == BOUND_BAIL_AFTER && __popcll(__ballot(need)) >= BOUND_BAIL_LANES) { need = true; break; }
            need = need || !(two_subset_bound(shape, tx.pl, full) >= lim);
        }
        const unsigned long long ml = __ballot(live && need), mt = __ballot(live);
        if ((threadIdx.x & 63u) == 0u) { atomicAdd(counters + PILOT_LISTED, (int32_t)__popcll(ml)); atomicAdd(counters + PILOT_SAMPLED, (int32_t)__popcll(mt)); }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(counters + PILOT_DONE, 1) == (int32_t)gridDim.x - 1) {  // the last workgroup: every count has arrived
            __threadfence();
            const int64_t listed = atomicAdd(counters + PILOT_LISTED, 0), sampled = atomicAdd(counters + PILOT_SAMPLED, 0);
            *flag = (listed * 256 <= (int64_t)thr256 * sampled) ? 1 : 0;
            if (host_counts) { host_counts[0] = (int32_t)listed; host_counts[1] = (int32_t)sampled; __threadfence_system(); }
        }
    }
}

// start of an RGB bounded call: the list lengths, the pilot's words and both bands' pair counters start at zero (`counters`: CTR_WORDS words, then
// PAIR_CTR_WORDS per band), and each band's PairTarget goes behind its pair counters
__global__ void __launch_bounds__(TPB) bc7_bounded_setup(int32_t* __restrict__ counters, const PairTarget t0, const PairTarget t1)
{
    for (int i = (int)threadIdx.x; i < CTR_WORDS + 2 * PAIR_CTR_WORDS; i += TPB) {
        const int j = i < CTR_WORDS ? 0 : (i - CTR_WORDS) % PAIR_CTR_WORDS;
        if (i < CTR_WORDS || j < PAIR_CTR_TARGET) counters[i] = 0;
    }
    if (threadIdx.x == 0) {
        *reinterpret_cast<PairTarget*>(counters + CTR_WORDS + PAIR_CTR_TARGET) = t0;
        *reinterpret_cast<PairTarget*>(counters + CTR_WORDS + PAIR_CTR_WORDS + PAIR_CTR_TARGET) = t1;
    }
}

// ---- PAIRS: the list scan of the RGB bounded order, cut down to the (block, shape) pairs the bound cannot exclude ---------------
// bc7_finish_all<3> lists a block as soon as ONE shape's two_subset_bound is below the incumbent `inc`; the list scan then fits all 64
// shapes of it, both modes.  On the bench surface 1.6 of a listed block's 64 shapes have a bound below inc (profiles/bc7_pair_survival.txt).
// A mode-1/3 encoding of shape s, fast or refined, has error >= LB(s), so with P1 = {s : LB(s) < inc - opaque - 0.5} (finish<3>'s rule):
//   * the reference refines s* = first strict minimum of the FAST error in rank order (kernel.ispc:1299-1363).  If s* is outside P1 the
//     mode cannot get below inc: it changes nothing.  If s* is in P1 it is also the ordered argmin over P1;
//   * so only "is the ordered argmin over P1 (fast error E1) really s*?" is open.  A shape outside P1 has fast error >= inc; it can
//     precede the P1 winner only if E1 >= inc.  E1 < inc: the P1 winner is s*, refined and committed as ever.  E1 >= inc: the P1 winner is
//     refined all the same; if that does not get below the live best error the mode changes nothing whichever shape s* is (s* = the P1
//     winner: the reference's refinement fails alike; s* outside P1: it cannot win).  Only where the refinement DOES get below although
//     E1 >= inc is the answer needed, and those few blocks take the full route: they go to a second list, the full list scan
//     (bc7_scan_all, split) and bc7_finish_all<4> run over it from the untouched incumbent.  Mode 3 is judged against the pre-mode-1 inc
//     (a superset of its own P1) and commits against the live best error.
// Three steps, per band (a block's 64 bounds are evaluated once: a separate builder kernel behind finish<3> used to evaluate them again):
//   bc7_finish_all<3> with the pair route on, its bound loop bounds every shape for every lane (no early exit and no bail: a listed
//                    block needs all 64 answers, and a wave that bailed would have to send 64 blocks through the full list scan, which
//                    costs more than the 60 bounds it saves) and keeps a bit per shape.  Behind the list append (the list position is
//                    the block's slot) it clears the block's two merged words and appends the survivors to one bucket per shape --
//                    counted per workgroup in LDS, one atomic per (workgroup, shape) -- so that every wave of the scan is shape-uniform
//                    (scalar subset masks).  Blocks with more than 32 survivors go to the second list at once;
//   bc7_pair_scan    lanes = pairs of one shape, grid-stride over wave tiles of 64 pairs: search_two_subset over that one shape, its
//                    rank key, and the ordered argmin (error, then key; keys are distinct) as a 64-bit atomicMin of (error << 32 | key)
//                    into one word per (listed block, mode) -- no share table, no merge;
//   bc7_finish_all<8> reads the words, refines, commits or defers the block to the second list.
// A bucket that overflows (photograph-like content that slipped past the pilot: nearly every shape survives) raises the band's overflow
// word: the pair scan returns at once and finish<8> defers every listed block, i.e. the band runs the full list scan.  Same bytes.

__global__ void __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(4, 4)))
bc7_pair_scan(const uint8_t* __restrict__ src, int64_t stride, int32_t blocks_x, const int32_t* __restrict__ list, const uint4* __restrict__ compact,
              const bc7_enc_settings S, const PairRegion P)
{
    __shared__ unsigned short s_seed16[2048];
    __shared__ uint32_t s_seed32[2048];
    __shared__ uint2 s_pal[12 * TPB];                               // 8 + 4 levels per lane, as in the table-order scans
    __shared__ int32_t s_first[65];                                 // first wave tile of each shape's bucket
    if (P.ctr[PAIR_CTR_OVERFLOW]) return;                           // whole grid: the builder finished before this launch
    if (threadIdx.x == 0) {
        int32_t t = 0;
        for (int s = 0; s < 64; s++) { s_first[s] = t; t += (P.ctr[s] + 63) >> 6; }
        s_first[64] = t;
    }
    __syncthreads();
    const int32_t total = s_first[64];
    const int32_t wpb = TPB / 64;
    if ((int32_t)blockIdx.x * wpb >= total) return;                 // whole workgroup: no barrier is pending
    Lane ln;
    ln.T = stage_seed_tables_fast(s_seed16, s_seed32, threadIdx.x, TPB);
    __syncthreads();
    ln.keys = nullptr;
    ln.pal = s_pal + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    const bool on_a = S.fastSkipTreshold_mode1 > 0, on_b = S.fastSkipTreshold_mode3 > 0;
    int shape = 0;
#pragma unroll 1
    for (int32_t tile = (int32_t)blockIdx.x * wpb + (int32_t)(threadIdx.x >> 6); tile < total; tile += (int32_t)gridDim.x * wpb) {
        while (s_first[shape + 1] <= tile) shape++;                  // tiles grow along the loop: the search never goes back
        shape = __builtin_amdgcn_readfirstlane(shape);               // wave-uniform: subset masks stay scalars
        const int32_t len = P.ctr[shape];
        const int32_t at = (tile - s_first[shape]) * 64 + lane;
        const bool live = at < len;
        const int32_t slot = P.buckets[(int64_t)shape * P.cap + (live ? at : len - 1)];   // idle lanes redo the bucket's last pair, merge nothing
        if (compact) load_block_compact(ln.tx, compact, slot); else load_block<false>(ln.tx, src, stride, blocks_x, list[slot]);
        // the table-order scan's own code for exactly one shape (first = shape, step = 64): the fast errors of modes 1 / 3 ...
        Win wa, wb;
        search_two_subset<false, 3, 0>(ln, S, wa, wb, shape, 64);
        const int32_t ea = wa.err, ec = wb.err;
        // ... and the shape's rank key, which orders equal errors (the scan evaluates it on a tie only; here every pair carries it)
        ln.tx.fence();
        Stats<3> rfull;
        whole_block_rank_stats<3, 3>(rfull, ln.tx);
        const uint32_t key = (uint32_t)rank_key<3>(shape, ln.tx, rfull, ln.T);
        if (live && on_a) atomicMin(reinterpret_cast<unsigned long long*>(P.words + 2 * (int64_t)slot),     ((unsigned long long)(uint32_t)ea << 32) | key);
        if (live && on_b) atomicMin(reinterpret_cast<unsigned long long*>(P.words + 2 * (int64_t)slot + 1), ((unsigned long long)(uint32_t)ec << 32) | key);
    }
}

// ---- ROT TASKS: modes 4/5 of the RGB bounded order for the (block, rotation) pairs a bound leaves (round 9) ----------------------
// bc7_finish_all<3> runs the nine mode 4/5 candidates of every block (3 rotations x {mode 4, mode 4 swapped, mode 5}): 15 % of a `slow`
// call's instructions.  Under an RGB profile every candidate of rotation p has error >= rotation_bound(p) (bc7_exact.hpp), and modes 4/5
// replace the block only below the error e02 modes 0/2 left: on the bench surface 0.565 of the (block, rotation) pairs survive, on a
// photograph 0.81 (profiles/r09_bc7_rotation_survival.txt) -- but no whole wave of blocks agrees, so finish<3> cannot skip in place.
// As for the pairs of modes 1/3, the survivors are listed and full waves run over the lists.  finish<3> becomes three launches per band:
//   bc7_finish_all<9>   modes 0/2 refined, the block stored, inc_err = e02, the block's merged word emptied, and the block appended to
//                       the list of each surviving rotation (one list per rotation: the task kernel's waves stay rotation-uniform);
//   bc7_rot_tasks       lanes = entries of one rotation list, wave tiles walked by the device-side counts.  The rotation's three
//                       candidates run through modes_45_scan from bound = e02 -- the arithmetic of the inline route -- and the task
//                       publishes at most ONE candidate, strictly below e02: its mode 5 if that is strictly below its mode 4, else its
//                       mode 4.  The reference's result after modes 4 and 5 is the first strict minimum over [mode 4: r0 s0, r0 s1, r1 s0,
//                       ...; then mode 5: r0, r1, r2] (kernel.ispc:1623-1655): a task whose mode 5 does not beat its own mode 4 cannot
//                       supply the winner with mode 5 (mode 4's minimum over all rotations is lower still), and one whose mode 5 does
//                       cannot supply it with mode 4.  The emitted block goes to payload slot (rotation, list position), and a 64-bit
//                       atomicMin of the merged word (RotRegion) settles the rest: lowest error, then mode 4, then the lower rotation;
//   bc7_finish_all<10>  admits the word's candidate with a strict `<`, runs mode 6 in its place, leaves the incumbent of modes 1/3 in inc_err;
//   bc7_bound_list      (round 11) finish<3>'s tail from that incumbent, unchanged: one device function (bounded_list_tail) for both.
// A rotation the bound excludes cannot get below e02, so it can neither win nor, by a tie, displace a winner: same bytes.
// ITW_BC7_ROT_TASKS=0 (read at every call): finish<3> as before.
// Two waves per SIMD: 246 VGPRs, nothing spilled.  At three (168 VGPRs) 38 registers spill and the call is 1.2 % slower (4.29 against 4.24 ms on
// the bench surface): the call pays for instructions, and the other band's kernels fill the SIMDs anyway.
#ifndef ROT_TASK_WAVES
#define ROT_TASK_WAVES 2
#endif
template <bool VEC16>
__global__ void __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(ROT_TASK_WAVES, ROT_TASK_WAVES)))
bc7_rot_tasks(const uint8_t* __restrict__ src, int64_t stride, int32_t blocks_x, const bc7_enc_settings S, const int32_t* __restrict__ inc_err, const RotRegion R)
{
    __shared__ unsigned short s_seed16[2048];
    __shared__ uint32_t s_seed32[2048];
    __shared__ uint2 s_pal[8 * TPB];                                // a candidate's vector palette (<= 8 levels), then its scalar levels
    __shared__ int32_t s_first[4];                                  // first wave tile of each rotation's list
    if (threadIdx.x == 0) {
        int32_t t = 0;
        for (int r = 0; r < 3; r++) { s_first[r] = t; t += (R.counts[r] + 63) >> 6; }
        s_first[3] = t;
    }
    __syncthreads();
    const int32_t total = s_first[3];
    const int32_t wpb = TPB / 64;
    if ((int32_t)blockIdx.x * wpb >= total) return;                 // whole workgroup: no barrier is pending (empty lists: the other order, or nothing survives)
    Lane ln;
    ln.T = stage_seed_tables_fast(s_seed16, s_seed32, threadIdx.x, TPB);
    __syncthreads();
    ln.keys = nullptr;
    ln.pal = s_pal + threadIdx.x;
    ln.best_err = ERR_MAX; ln.improved = false; ln.opaque_err = 0;
    ln.best[0] = ln.best[1] = ln.best[2] = ln.best[3] = 0u;
    const int lane = (int)(threadIdx.x & 63u);
    const int32_t first1 = s_first[1], first2 = s_first[2];
#pragma unroll 1
    for (int32_t tile = (int32_t)blockIdx.x * wpb + (int32_t)(threadIdx.x >> 6); tile < total; tile += (int32_t)gridDim.x * wpb) {
        const int r = __builtin_amdgcn_readfirstlane((tile >= first1 ? 1 : 0) + (tile >= first2 ? 1 : 0));   // wave-uniform
        const int32_t len = R.counts[r];
        const int32_t at = (tile - s_first[r]) * 64 + lane;
        const bool live = at < len;
        const int32_t pos = live ? at : len - 1;                    // idle lanes redo the list's last block, publish nothing
        const int32_t b = R.lists[(int64_t)r * R.cap + pos];
        load_block<VEC16>(ln.tx, src, stride, blocks_x, b);
        const int32_t inc = inc_err[b];
        Dual best4, best5;
        clear(best4); clear(best5);
        int32_t err4 = inc, err5 = ERR_MAX;
        modes_45_scan(ln, S, r, r + 1, best4, err4, best5, err5);
        const bool five = err5 < err4;                              // err4 <= inc: strictly below the incumbent either way
        if (five || err4 < inc) {
            uint32_t blk[4] = {0u, 0u, 0u, 0u};
            if (five) emit_dual<5>(blk, best5); else emit_dual<4>(blk, best4);
            if (live) {
                R.payload[(int64_t)r * R.cap + pos] = make_uint4(blk[0], blk[1], blk[2], blk[3]);
                const unsigned long long word = ((unsigned long long)(uint32_t)(five ? err5 : err4) << 32) | ((five ? 1ull : 0ull) << ROT_WORD_MODE5_SHIFT) |
                                                ((unsigned long long)r << ROT_WORD_ROT_SHIFT) | (unsigned long long)pos;
                atomicMin(R.words + b, word);
            }
        }
        ln.tx.fence();
    }
}

// ---- WIDE path: calls too small to fill the chip -----------------------------------------------------------------
// The kernels above give every block one lane and every mode family its own pair of launches, which is what fills
// 1024 SIMDs for a whole surface -- and what makes a 16 384-block call (the plugin's 0x40000-pixel slice,
// IntelPlugin.cpp:851) take a millisecond: 256 waves walk through five dependent launches while three quarters of the
// chip idle.  The reference's own answer to small work items is to cut them into bands for more threads
// (win32Threads.cpp:211-249); the GPU-side equivalent cuts the *search* instead:
//   phase 1  one launch whose blockIdx.y enumerates independent tasks -- the scan of each multi-subset family split
//            into `parts` strided shares of its candidate list (lanes stay blocks; another wave takes the other shapes).
//            A split scan leaves one winner per (mode, part).  Register budget of the scans: 4 waves per SIMD;
//   phase 2  one launch, blockIdx.y = task: per multi-subset mode an ORDERED ARGMIN over the parts' winners -- lowest
//            error, then the reference's strict-`<` tie rule (lowest table index for modes 0/2, lowest PCA rank key for
//            modes 1/3/7, kernel.ispc:1320, 1348, 1404-1409; keys are evaluated only on a tie) -- then the least-squares
//            refinement; next to them one task per mode 4/5 rotation and one for mode 6 (2 waves per SIMD);
//   phase 3  the modes' candidates {error, block} compete in the reference's order 0,2,1,3,7,4,5,6 with strict `<`
//            (kernel.ispc:1970-1977).
// Every candidate is evaluated by exactly the code of the deep path (same functions, same arithmetic), only by a different
// wave, so the emitted block is identical; tests run both paths on the same inputs (ITW_BC7_PATH=deep|wide).
constexpr int WIDE_SLOTS = 18;            // candidate slots in commit order: m0 m2 m1 m3 m7 m4[r0..r3][swap 0,1] m5[r0..r3] m6
constexpr int WIDE_SLOT_M4 = 5, WIDE_SLOT_M5 = 13, WIDE_SLOT_M6 = 17;
constexpr int WIDE_MAX_TASKS = 56;
constexpr int WIDE_MAX_PARTS = 16;
struct WideTasks { int n; uint8_t kind[WIDE_MAX_TASKS]; uint8_t part[WIDE_MAX_TASKS]; uint8_t parts[WIDE_MAX_TASKS]; };
struct WideModes { int n; uint8_t mode[20]; uint8_t parts[20]; };    // mode: 0,2,1,3,7 refine | 100 + 4 r + c: rotation r, candidate c (mode 4, mode 4 swapped, mode 5) | 6


// winners of split scans: [win_slot][part][block] x {err, shape, key, -}, `pstride` parts per slot
struct WideDims { int32_t nblocks; int32_t pstride; };
__device__ __forceinline__ void store_win_wide(uint4* __restrict__ wins, WideDims d, int slot, int part, int32_t b, const Win& w)
{
    wins[((int64_t)slot * d.pstride + part) * d.nblocks + b] = make_uint4((uint32_t)w.err, (uint32_t)w.shape, (uint32_t)w.key, 0u);
}
__device__ __forceinline__ void load_win_wide(Win& w, const uint4* __restrict__ wins, WideDims d, int slot, int part, int32_t b)
{
    const uint4 v = wins[((int64_t)slot * d.pstride + part) * d.nblocks + b];
    w.err = (int32_t)v.x; w.shape = (int32_t)v.y; w.key = (int32_t)v.z;
}
__device__ __forceinline__ void store_candidate(int32_t* __restrict__ cerr, uint4* __restrict__ cblk, int32_t nblocks, int slot, int32_t b,
                                                int32_t err, const uint32_t (&blk)[4])
{
    cerr[(int64_t)slot * nblocks + b] = err;
    cblk[(int64_t)slot * nblocks + b] = make_uint4(blk[0], blk[1], blk[2], blk[3]);
}

// Ordered argmin over the parts of one mode's split scan.
template <int MODE>
__device__ __forceinline__ void merge_parts(Win& w, Lane& ln, const uint4* __restrict__ wins, WideDims dims, int parts, int32_t b, int channels)
{
    load_win_wide(w, wins, dims, wide_win_slot(MODE), 0, b);
    for (int p = 1; p < parts; p++) {
        Win x;
        load_win_wide(x, wins, dims, wide_win_slot(MODE), p, b);
        if (x.err < w.err) { w = x; continue; }
        if (x.err != w.err || x.err == ERR_MAX) continue;
        if (MODE == 0 || MODE == 2) {                     // table order: lowest shape index
            if (x.shape < w.shape) w = x;
        } else {                                          // PCA-ranked list order: lowest rank key
            if (MODE == 7) {
                if (channels == 4) { w.key = merge_key<4, 4>(w, ln.tx, ln.T); x.key = merge_key<4, 4>(x, ln.tx, ln.T); }
                else               { w.key = merge_key<4, 3>(w, ln.tx, ln.T); x.key = merge_key<4, 3>(x, ln.tx, ln.T); }
            } else { w.key = merge_key<3, 3>(w, ln.tx, ln.T); x.key = merge_key<3, 3>(x, ln.tx, ln.T); }
            if (x.key < w.key) w = x;
        }
    }
}

#ifndef WIDE_SCAN_WAVES
#define WIDE_SCAN_WAVES 4
#endif
// a scan is split until its waves fill 1 / WIDE_FILL_DIVISOR of the chip's wave slots (tuning constant, like the register budgets)
#ifndef WIDE_FILL_DIVISOR
#define WIDE_FILL_DIVISOR 2
#endif
// RANKED_LISTS: some family scans a PCA-ranked prefix (fast presets): that code keeps 16 sorted keys in registers and runs
// at 3 waves per SIMD like its deep counterpart; the whole-table instantiation (slow presets) compiles it out.
template <bool VEC16, bool RANKED_LISTS>
__global__ void __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(RANKED_LISTS ? 3 : WIDE_SCAN_WAVES, RANKED_LISTS ? 3 : WIDE_SCAN_WAVES)))
bc7_wide_phase1(const uint8_t* __restrict__ src, int64_t stride, int32_t blocks_x, int32_t nblocks, uint4* __restrict__ wins,
                int32_t* __restrict__ cerr, uint4* __restrict__ cblk, const bc7_enc_settings S, const WideTasks tasks, const int ranked13, const int ranked7,
                const int pstride)
{
    const WideDims dims{nblocks, pstride};
    __shared__ unsigned short s_seed16[2048];
    __shared__ uint32_t s_seed32[2048];
    __shared__ uint2 s_pal[(RANKED_LISTS ? 16 : 12) * TPB];
    Lane ln;
    ln.T = stage_seed_tables_fast(s_seed16, s_seed32, threadIdx.x, TPB);
    __syncthreads();
    const int32_t gid = blockIdx.x * TPB + threadIdx.x;
    const bool live = gid < nblocks;
    const int32_t b = live ? gid : nblocks - 1;
    ln.keys = nullptr;
    ln.pal = s_pal + threadIdx.x;
    load_block<VEC16>(ln.tx, src, stride, blocks_x, b);
    ln.best_err = ERR_MAX; ln.opaque_err = 0; ln.improved = false;
    ln.best[0] = ln.best[1] = ln.best[2] = ln.best[3] = 0u;

    const int kind = tasks.kind[blockIdx.y], part = tasks.part[blockIdx.y], parts = tasks.parts[blockIdx.y];   // wave-uniform
    if (kind == WK_SCAN02) {
        Win w0, w2;
        search_02(ln, S, w0, w2, part, parts);
        if (live) { store_win_wide(wins, dims, wide_win_slot(0), part, b, w0); if (!S.skip_mode2) store_win_wide(wins, dims, wide_win_slot(2), part, b, w2); }
    } else if (kind == WK_SCAN13) {
        Win w1, w3;
        if (RANKED_LISTS && ranked13) search_two_subset<false, 3, 2>(ln, S, w1, w3, part, parts); else search_two_subset<false, 3, 0>(ln, S, w1, w3, part, parts);
        if (live) { store_win_wide(wins, dims, wide_win_slot(1), part, b, w1); store_win_wide(wins, dims, wide_win_slot(3), part, b, w3); }
    } else {
        Win w7, unused;
        if (S.channels == 4) { if (RANKED_LISTS && ranked7) search_two_subset<true, 4, 2>(ln, S, w7, unused, part, parts); else search_two_subset<true, 4, 0>(ln, S, w7, unused, part, parts); }
        else                 { if (RANKED_LISTS && ranked7) search_two_subset<true, 3, 2>(ln, S, w7, unused, part, parts); else search_two_subset<true, 3, 0>(ln, S, w7, unused, part, parts); }
        if (live) store_win_wide(wins, dims, wide_win_slot(7), part, b, w7);
    }
}

// SINGLES = false: the refine tasks (modes 0,2,1,3,7; need phase 1).  SINGLES = true: the single-subset tasks (mode 4/5
// candidates, mode 6), which depend on nothing and run on a second stream beside phase 1 when the caller provides one.
template <bool VEC16, bool SINGLES>
// SINGLES (one mode 4/5 candidate group or mode 6 per wave, nothing else live): 168 VGPRs hold it with 10 cold spills, and 44 KiB of LDS let
// three workgroups share a CU: 3 waves per SIMD run modes 4/5 of a call 14 % faster than 2 (profiles/r06_modes45_mapping_probe.txt)
#ifndef WIDE_SINGLES_WAVES
#define WIDE_SINGLES_WAVES 3
#endif
__global__ void __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(SINGLES ? WIDE_SINGLES_WAVES : 2, SINGLES ? WIDE_SINGLES_WAVES : 2)))
bc7_wide_phase2(const uint8_t* __restrict__ src, int64_t stride, int32_t blocks_x, int32_t nblocks, const uint4* __restrict__ wins,
                int32_t* __restrict__ cerr, uint4* __restrict__ cblk, const bc7_enc_settings S, const WideModes modes, const int pstride)
{
    const WideDims dims{nblocks, pstride};
    __shared__ unsigned short s_seed16[2048];
    __shared__ uint32_t s_seed32[2048];
    __shared__ uint2 s_pal[(SINGLES ? 16 : LANE_PAL_LEVELS) * TPB];   // mode 4/5 vector part, mode 6 (16 levels) / refinement palettes
    Lane ln;
    ln.T = stage_seed_tables_fast(s_seed16, s_seed32, threadIdx.x, TPB);
    __syncthreads();
    const int32_t gid = blockIdx.x * TPB + threadIdx.x;
    const bool live = gid < nblocks;
    const int32_t b = live ? gid : nblocks - 1;
    ln.keys = nullptr;
    ln.pal = s_pal + threadIdx.x;
    load_block<VEC16>(ln.tx, src, stride, blocks_x, b);
    ln.best_err = ERR_MAX; ln.improved = false;
    ln.best[0] = ln.best[1] = ln.best[2] = ln.best[3] = 0u;
    ln.opaque_err = 0;                                                             // kernel.ispc:1267-1277
    if (S.channels == 4) {
        uint32_t e = 0;
#pragma unroll
        for (int d = 0; d < 4; d++) { const uint32_t x = ~ln.tx.pl[3][d]; e = udot4(x, x, e); }
        ln.opaque_err = (int32_t)e;
    }
    const int mode = modes.mode[blockIdx.y], parts = modes.parts[blockIdx.y];      // wave-uniform
    if (SINGLES && mode >= 100) {                                                  // one mode 4/5 candidate of one rotation
        const int r = (mode - 100) >> 2, c = (mode - 100) & 3;
        Dual best4, best5;
        clear(best4); clear(best5);
        int32_t err4 = ERR_MAX, err5 = ERR_MAX;
        modes_45_scan(ln, S, r, r + 1, best4, err4, best5, err5, c == 3 ? 7 : 1 << c);       // c == 3: all three in this wave
        uint32_t blk[4] = {0u, 0u, 0u, 0u};
        if (c != 2) {                                     // mode 4 (c == 3: the better of both swaps, first wins a tie: slot of swap 0)
            if (err4 < ERR_MAX) emit_dual<4>(blk, best4);
            if (live) store_candidate(cerr, cblk, nblocks, WIDE_SLOT_M4 + 2 * r + (c == 1 ? 1 : 0), b, err4, blk);
        }
        if (c >= 2) {
            blk[0] = blk[1] = blk[2] = blk[3] = 0u;
            if (err5 < ERR_MAX) emit_dual<5>(blk, best5);
            if (live) store_candidate(cerr, cblk, nblocks, WIDE_SLOT_M5 + r, b, err5, blk);
        }
        return;
    }
    if (SINGLES) {                                                                 // mode 6
        if (S.channels == 4) mode_6<4>(ln, S); else mode_6<3>(ln, S);
        if (live) store_candidate(cerr, cblk, nblocks, WIDE_SLOT_M6, b, ln.best_err, ln.best);
        return;
    }
    Win w;
    int slot = 0;
    if (mode == 0)      { merge_parts<0>(w, ln, wins, dims, parts, b, S.channels); refine_and_commit<0>(ln, w, S.refineIterations[0], S.channels); slot = 0; }
    else if (mode == 2) { merge_parts<2>(w, ln, wins, dims, parts, b, S.channels); refine_and_commit<2>(ln, w, S.refineIterations[2], S.channels); slot = 1; }
    else if (mode == 1) { merge_parts<1>(w, ln, wins, dims, parts, b, S.channels); refine_and_commit<1>(ln, w, S.refineIterations[1], S.channels); slot = 2; }
    else if (mode == 3) { merge_parts<3>(w, ln, wins, dims, parts, b, S.channels); refine_and_commit<3>(ln, w, S.refineIterations[3], S.channels); slot = 3; }
    else                { merge_parts<7>(w, ln, wins, dims, parts, b, S.channels); refine_and_commit<7>(ln, w, S.refineIterations[7], S.channels); slot = 4; }
    if (live) store_candidate(cerr, cblk, nblocks, slot, b, ln.best_err, ln.best);
}

__global__ void __launch_bounds__(TPB)
bc7_wide_commit(const int32_t* __restrict__ cerr, const uint4* __restrict__ cblk, int32_t nblocks, uint32_t active_slots, uint4* __restrict__ dst, int vec16)
{
    const int32_t b = blockIdx.x * TPB + threadIdx.x;
    if (b >= nblocks) return;
    int32_t best = ERR_MAX;
    uint4 blk = make_uint4(0u, 0u, 0u, 0u);
    for (int slot = 0; slot < WIDE_SLOTS; slot++) {
        if (!((active_slots >> slot) & 1u)) continue;
        const int32_t e = cerr[(int64_t)slot * nblocks + b];
        if (e < best) { best = e; blk = cblk[(int64_t)slot * nblocks + b]; }
    }
    if (vec16) dst[b] = blk;
    else { uint32_t* d = reinterpret_cast<uint32_t*>(dst) + (int64_t)b * 4; d[0] = blk.x; d[1] = blk.y; d[2] = blk.z; d[3] = blk.w; }
}

struct Bc7Launch {
    bool vec; dim3 grid; hipStream_t st; const uint8_t* src; int64_t stride; int bx; int32_t n;
    uint8_t* dst; int32_t* err; uint4* wins; bc7_enc_settings S; int first;
};

// A runtime bool as a std::bool_constant for a generic lambda: a kernel launch is written once, and both of its instances exist.
template <class F> static void with_bool(bool b, F&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
template <class F> static void with_bools(bool a, bool b, F&& f) { with_bool(a, [&](auto A) { with_bool(b, [&](auto B) { f(A, B); }); }); }

template <int FAMILY, int RANKED>
static void launch_search(const Bc7Launch& L)
{
    const size_t lds = RANKED == 1 ? (size_t)64 * TPB * sizeof(int32_t) : 0;
    with_bool(L.vec, [&](auto V) { hipLaunchKernelGGL((bc7_search_kernel<FAMILY, RANKED, decltype(V)::value>), L.grid, dim3(TPB), lds, L.st, L.src, L.stride, L.bx, L.n, L.wins, L.S); });
}
template <int FAMILY>
static void launch_finish(Bc7Launch& L)
{
    with_bool(L.vec, [&](auto V) { hipLaunchKernelGGL((bc7_finish_kernel<FAMILY, decltype(V)::value>), L.grid, dim3(TPB), 0, L.st, L.src, L.stride, L.bx, L.n, L.dst, L.err, L.wins, L.S, L.first); });
    L.first = 0;
}

// Calls of at most this many blocks take the wide path (measured crossover on MI355X, tools/bc7_path_probe.py).
#ifndef ITW_BC7_WIDE_MAX_BLOCKS
#define ITW_BC7_WIDE_MAX_BLOCKS 262144
#endif

#ifdef ITW_TEST_HOOKS
// test hook (itwTestBc7TwoSubsetBounds, libispc_texcomp_test.so only): two_subset_bound of every two-subset shape of every block, out[block * 64 + shape]
template <bool VEC16>
__global__ void __launch_bounds__(TPB) bc7_test_bounds(const uint8_t* __restrict__ src, int64_t stride, int32_t blocks_x, int32_t nblocks, float* __restrict__ out)
{
    const int32_t gid = blockIdx.x * TPB + threadIdx.x;
    const int32_t b = gid < nblocks ? gid : nblocks - 1;
    Tex tx;
    load_block<VEC16>(tx, src, stride, blocks_x, b);
    IStats<3> full;
    stats_int<3>(full, tx.pl, whole_block());
#pragma unroll 1
    for (int shape = 0; shape < 64; shape++) {
        const float lb = two_subset_bound(shape, tx.pl, full);
        if (gid < nblocks) out[(int64_t)b * 64 + shape] = lb;
    }
}
void launch_bc7_test_bounds(const uint8_t* src, int64_t stride, int width, int height, float* out, hipStream_t st)
{
    const int bx = width / 4;
    const int64_t n = (int64_t)bx * (height / 4);
    if (n <= 0) return;
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride) & 15) == 0;
    const dim3 grid((unsigned)((n + TPB - 1) / TPB));
    with_bool(vec, [&](auto V) { hipLaunchKernelGGL((bc7_test_bounds<decltype(V)::value>), grid, dim3(TPB), 0, st, src, stride, bx, (int32_t)n, out); });
}
// test hook (itwTestBc7RotationBounds): rotation_bound of the three rotations of every block, out[block * 3 + rotation]
template <bool VEC16>
__global__ void __launch_bounds__(TPB) bc7_test_rot_bounds(const uint8_t* __restrict__ src, int64_t stride, int32_t blocks_x, int32_t nblocks, float* __restrict__ out)
{
    const int32_t gid = blockIdx.x * TPB + threadIdx.x;
    const int32_t b = gid < nblocks ? gid : nblocks - 1;
    Tex tx;
    load_block<VEC16>(tx, src, stride, blocks_x, b);
    IStats<3> full;
    stats_int<3>(full, tx.pl, whole_block());
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float lb = rotation_bound(r, full);
        if (gid < nblocks) out[(int64_t)b * 3 + r] = lb;
    }
}
void launch_bc7_test_rot_bounds(const uint8_t* src, int64_t stride, int width, int height, float* out, hipStream_t st)
{
    const int bx = width / 4;
    const int64_t n = (int64_t)bx * (height / 4);
    if (n <= 0) return;
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride) & 15) == 0;
    const dim3 grid((unsigned)((n + TPB - 1) / TPB));
    with_bool(vec, [&](auto V) { hipLaunchKernelGGL((bc7_test_rot_bounds<decltype(V)::value>), grid, dim3(TPB), 0, st, src, stride, bx, (int32_t)n, out); });
}
// test hook (itwTestBc7F02Scan): search_02 of every block twice -- in the scheduled order with both caches, as the head scan runs it, and in
// table order with nothing cached.  out[(block * 2 + order) * 84 + ..]: mode 0's winner (error, shape), mode 2's winner (error, shape), the
// 16 mode 0 and the 64 mode 2 errors by table index.  The winners alone would hide a stale slot wherever the wrong value does not win.
template <bool VEC16>
__global__ void __launch_bounds__(TPB) bc7_test_f02_scan(const uint8_t* __restrict__ src, int64_t stride, int32_t blocks_x, int32_t nblocks, int32_t* __restrict__ out)
{
    __shared__ unsigned short s_seed16[2048];
    __shared__ uint32_t s_seed32[2048];
    __shared__ uint2 s_pal[14 * TPB];
    Lane ln;
    ln.T = stage_seed_tables_fast(s_seed16, s_seed32, threadIdx.x, TPB);
    __syncthreads();
    const int32_t gid = blockIdx.x * TPB + threadIdx.x;
    const bool live = gid < nblocks;
    const int32_t b = live ? gid : nblocks - 1;
    ln.keys = nullptr;
    ln.pal = s_pal + threadIdx.x;
    load_block<VEC16>(ln.tx, src, stride, blocks_x, b);
    bc7_enc_settings S = {};                                        // search_02 reads skip_mode2 alone
    int32_t* const o = live ? out + (int64_t)b * 168 : nullptr;
    Win w0, w2;
    search_02<true, true>(ln, S, w0, w2, 0, 1, live ? o + 4 : nullptr);
    if (live) { o[0] = w0.err; o[1] = w0.shape; o[2] = w2.err; o[3] = w2.shape; }
    search_02<false, false>(ln, S, w0, w2, 0, 1, live ? o + 88 : nullptr);
    if (live) { o[84] = w0.err; o[85] = w0.shape; o[86] = w2.err; o[87] = w2.shape; }
}
void launch_bc7_test_f02_scan(const uint8_t* src, int64_t stride, int width, int height, int32_t* out, hipStream_t st)
{
    const int bx = width / 4;
    const int64_t n = (int64_t)bx * (height / 4);
    if (n <= 0) return;
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride) & 15) == 0;
    const dim3 grid((unsigned)((n + TPB - 1) / TPB));
    with_bool(vec, [&](auto V) { hipLaunchKernelGGL((bc7_test_f02_scan<decltype(V)::value>), grid, dim3(TPB), 0, st, src, stride, bx, (int32_t)n, out); });
}
// test hook (itwTestBc7RouteCounters): the route witness -- what ITW_ROUTE_SEEN counts, here and in abi.hip's launch()
static std::atomic<long long> g_route_seen[ITW_ROUTE_COUNTERS];
void bc7_route_seen(int what) { g_route_seen[what].fetch_add(1, std::memory_order_relaxed); }
void bc7_route_counters(int64_t* out, int n)
{
    for (int i = 0; i < n && i < ITW_ROUTE_COUNTERS; i++) out[i] = g_route_seen[i].load(std::memory_order_relaxed);
}
void bc7_route_counters_reset()
{
    for (int i = 0; i < ITW_ROUTE_COUNTERS; i++) g_route_seen[i].store(0, std::memory_order_relaxed);
}
// test hook (itwTestBc7CallCounters): what the last call of the RGB bounded order counted on the device (launch_rgb_bounded snapshots it
// while armed; it synchronises)
static std::atomic<int> g_counters_armed{0};
static std::atomic<int32_t> g_call_counters[ITW_BC7_CALL_COUNTERS];
void bc7_arm_call_counters(int on) { g_counters_armed.store(on ? 1 : 0, std::memory_order_relaxed); }
void bc7_call_counters(int32_t* out, int n)
{
    for (int i = 0; i < n && i < ITW_BC7_CALL_COUNTERS; i++) out[i] = g_call_counters[i].load(std::memory_order_relaxed);
}
#endif // ITW_TEST_HOOKS

// ---- the environment switches: one table, one reader -------------------------------------------------------------------------
//   ITW_BC7_PATH=deep|wide    force a path (tests and probes; itwSetBc7Path overrides it)
//   ITW_STAGED_BANDS=0        the staged runs of a host-pointer call do not run as overlapped deep bands
//   ITW_BC7_BOUND=0           modes 1/3 in the reference's place instead of last-and-bounded (same bytes; tools/gpu_env_matrix.sh runs both)
//   ITW_BC7_PILOT_THR=<pct>   the pilot's threshold (bc7_pilot_threshold; itwSetBc7Pilot overrides it)
//   ITW_BC7_PILOT_DEBUG=1     print the pilot's, the pair route's and the rotation lists' counters after a two-band call
//   ITW_BC7_BANDS=1           one band on the caller's stream, no pilot (round 4's launch order); default 2
//   ITW_BC7_COMPACT=0         the list scans gather their blocks from the surface (round 4) instead of reading the compact copy
//   ITW_BC7_FUSED=0           the per-family kernels instead of the two-launch fused shape
//   ITW_BC7_ALPHA_PRUNE=0     RGBA profiles: always the reference's order
//   ITW_BC7_PAIRS=0           the RGB bounded order's list scan fits all 64 shapes of every listed block (round 4) instead of the (block, shape)
//                             pairs the bound leaves (bc7_pair_scan's header)
//   ITW_BC7_PAIR_CAP=<n>      lowers a shape bucket's capacity (never raises it): a small value forces the overflow route
//   ITW_BC7_ROT_TASKS=0       modes 4/5 of the RGB bounded order inline in bc7_finish_all<3>, all nine candidates of every block, instead of the
//                             (block, rotation) pairs a bound leaves (bc7_rot_tasks' header)
// env_once: the process's first read holds (the workspace layout and the launch shape of later calls may depend on it).
// env_every_call: read again at every call -- PAIRS, PAIR_CAP and ROT_TASKS, on which the workspace layout does not depend, so that one process
// (the tests) can compare the routes.
enum EnvKind { ENV_OFF_AT_0, ENV_ON_AT_1, ENV_NUMBER, ENV_PATH_NAME };
enum EnvKey { ENV_PATH, ENV_STAGED_BANDS, ENV_BOUND, ENV_PILOT_THR, ENV_PILOT_DEBUG, ENV_BANDS, ENV_COMPACT, ENV_FUSED, ENV_ALPHA_PRUNE, ENV_PAIRS, ENV_PAIR_CAP,
              ENV_ROT_TASKS, ENV_KEYS };
#ifndef ITW_BC7_PILOT_THR_DEFAULT
#define ITW_BC7_PILOT_THR_DEFAULT 90     // forced either way by content (profiles/history/r05/r05l_*): 74 % estimated -> bounded wins by 11 %, 91 % -> equal, 98 % -> reference order by 0.6 %
#endif
struct EnvSwitch { const char* name; EnvKind kind; long unset; };
static constexpr EnvSwitch ENV_SWITCHES[ENV_KEYS] = {
    {"ITW_BC7_PATH", ENV_PATH_NAME, 0},      {"ITW_STAGED_BANDS", ENV_OFF_AT_0, 1}, {"ITW_BC7_BOUND", ENV_OFF_AT_0, 1},
    {"ITW_BC7_PILOT_THR", ENV_NUMBER, ITW_BC7_PILOT_THR_DEFAULT},                   {"ITW_BC7_PILOT_DEBUG", ENV_ON_AT_1, 0},
    {"ITW_BC7_BANDS", ENV_NUMBER, 2},        {"ITW_BC7_COMPACT", ENV_OFF_AT_0, 1},  {"ITW_BC7_FUSED", ENV_OFF_AT_0, 1},
    {"ITW_BC7_ALPHA_PRUNE", ENV_OFF_AT_0, 1}, {"ITW_BC7_PAIRS", ENV_OFF_AT_0, 1},   {"ITW_BC7_PAIR_CAP", ENV_NUMBER, 0},
    {"ITW_BC7_ROT_TASKS", ENV_OFF_AT_0, 1},
};
static long env_every_call(EnvKey k)
{
    const EnvSwitch& sw = ENV_SWITCHES[k];
    const char* e = std::getenv(sw.name);
    if (!e) return sw.unset;
    if (sw.kind == ENV_NUMBER) return std::atol(e);
    if (sw.kind == ENV_PATH_NAME) return !std::strcmp(e, "deep") ? 1 : !std::strcmp(e, "wide") ? 2 : 0;
    return sw.kind == ENV_OFF_AT_0 ? e[0] != '0' : e[0] == '1';
}
static long env_once(EnvKey k)
{
    static std::atomic<long long> seen[ENV_KEYS];                // 0 = not read yet, else value * 2 + 1
    long long v = seen[k].load(std::memory_order_relaxed);
    if (v == 0) seen[k].store(v = (long long)env_every_call(k) * 2 + 1, std::memory_order_relaxed);
    return (long)((v - 1) / 2);
}

// 0 = by size, 1 = deep always, 2 = wide whenever it supports the settings (itwSetBc7Path / ITW_BC7_PATH=deep|wide: tests and probes)
static std::atomic<int> g_bc7_path{-1};            // -1 = not set: the environment's
static int bc7_path_override()
{
    const int v = g_bc7_path.load(std::memory_order_relaxed);
    return v < 0 ? (int)env_once(ENV_PATH) : v;
}
void set_bc7_path(int v) { g_bc7_path.store(v == 1 || v == 2 ? v : 0, std::memory_order_relaxed); }
bool bc7_staged_bands_ok() { return env_once(ENV_STAGED_BANDS) && bc7_path_override() != 2; }

// Round 5.  ITW_BC7_PILOT_THR: the pilot's threshold in percent of the blocks it looks at that its estimate lists for modes 1/3 -- at or below it the rest of
// the surface takes the bounded order, above it the reference's; -1 = no pilot (always bounded), 0 = pilot, always the reference's order for the
// rest, 100 = pilot, always bounded (tools/order_timing.py under each setting: profiles/history/r05/r05e_*).  Returned in 1/256.
static std::atomic<int> g_bc7_pilot{-2};           // percent; -2 = not set: the environment's
static int bc7_pilot_threshold()
{
    const int set = g_bc7_pilot.load(std::memory_order_relaxed);
    const long pct = set == -2 ? env_once(ENV_PILOT_THR) : set;
    return pct < 0 ? -1 : (int)(pct > 100 ? 100 : pct) * 256 / 100;
}
void set_bc7_pilot(int percent) { g_bc7_pilot.store(percent < -1 ? -2 : (percent > 100 ? 100 : percent), std::memory_order_relaxed); }   // < -1: back to ITW_BC7_PILOT_THR / the default
static int bc7_bands() { return env_once(ENV_BANDS) < 2 ? 1 : 2; }
static int32_t bc7_pair_cap(int32_t layout_cap)
{
    const long v = env_every_call(ENV_PAIR_CAP);
    return (v > 0 && v < layout_cap) ? (int32_t)v : layout_cap;
}

// ---- what a call's settings switch on: read once, here ---------------------------------------------------------------------------
// A list length (fastSkipTreshold_mode*) is RANKED when it is a proper prefix of the shape ranking (1..63: the scan computes the 64 keys and
// fits the best few); LONG when it is ranked and longer than 16 (the keys then live in 64 KiB of LDS: the per-family kernels only).
// The three orders a call can take instead of the reference's {0,2} -> {1,3} -> {7} -> {4,5} -> {6}:
//   alpha_first  RGBA profile with both groups of modes: the alpha-capable modes first, the three-channel modes skipped where they cannot win
//                (bc7_finish_all's header)
//   bounded      modes 1/3 last and only where an exact bound cannot exclude them: profiles whose modes 1/3 scan every shape -- a ranked list
//                already spends a bound's worth of arithmetic per shape on its keys and then fits a few shapes only
//   rgb_bounded  the bounded order of the RGB profiles (`slow`): the one with bands' pair and rotation routes and a pilot's verdict
struct Bc7Modes {
    bool on02, on13, on7, on45, on6;
    bool r13, r7, long13, long7;
    int len1, len3, len7, channels;
    bool alpha_first, bounded, rgb_bounded;
    bool any() const { return on02 || on13 || on7 || on45 || on6; }
};
static Bc7Modes bc7_modes(const bc7_enc_settings& S)
{
    auto ranked = [](int t) { return t > 0 && t < 64; };
    Bc7Modes M;
    M.channels = S.channels == 4 ? 4 : 3;
    M.len1 = S.fastSkipTreshold_mode1; M.len3 = S.fastSkipTreshold_mode3; M.len7 = S.fastSkipTreshold_mode7;
    M.on02 = S.mode_selection[0]; M.on45 = S.mode_selection[2]; M.on6 = S.mode_selection[3];
    M.on13 = S.mode_selection[1] && (M.len1 > 0 || M.len3 > 0);
    M.on7 = S.mode_selection[1] && M.len7 > 0;
    M.r13 = M.on13 && (ranked(M.len1) || ranked(M.len3));
    M.long13 = M.r13 && (M.len1 > 16 || M.len3 > 16);
    M.r7 = M.on7 && ranked(M.len7);
    M.long7 = M.r7 && M.len7 > 16;
    M.alpha_first = env_once(ENV_ALPHA_PRUNE) && M.channels == 4 && (M.on02 || M.on13) && (M.on7 || M.on45 || M.on6);
    M.bounded = env_once(ENV_BOUND) && M.on02 && M.on13 && !M.r13;
    M.rgb_bounded = M.bounded && !M.alpha_first && !M.on7;
    return M;
}

// Above this many blocks an alpha-first call takes the fused shape even where the wide one is allowed: on translucent
// content it is 1.3-2.3x faster from 65536 blocks up, on opaque content (nothing to skip) at most 8 % slower from here
// (tools/bc7_path_probe.py, profiles/r02c_bc7_path_probe.txt vs r02b: alpha_basic 131072 blocks 0.361 / 0.758 vs 0.681 ms wide)
#define ITW_BC7_WIDE_MAX_BLOCKS_ALPHA_FIRST 131072

// the most blocks a call may have to take the wide path (-1: none): the forced path, else the caller's limit (0 = the library's), within the
// workspace bound of the wide layout (1.6 GB)
static int64_t bc7_wide_block_limit(int64_t wide_max)
{
    const int64_t hard_cap = (int64_t)1 << 20;
    const int o = bc7_path_override();
    if (o == 1) return -1;
    if (o == 2) return hard_cap;
    const int64_t limit = wide_max > 0 ? wide_max : ITW_BC7_WIDE_MAX_BLOCKS;
    return limit < hard_cap ? limit : hard_cap;
}
static bool bc7_use_wide(int64_t n, const bc7_enc_settings& S, const Bc7Modes& M, int64_t wide_max)
{
    // the wide ranked scan keeps the 16 smallest keys in registers: a family with a ranked list needs all its lists <= 16
    const bool lists_ok = !M.long13 && !M.long7;
    const bool rotations_ok = S.mode45_channel0 >= 0 && S.mode45_channel0 <= 3;
    const bool fused_pays = bc7_path_override() == 0 && n >= ITW_BC7_WIDE_MAX_BLOCKS_ALPHA_FIRST && M.alpha_first;     // (where the size decides)
    return lists_ok && rotations_ok && !fused_pays && n <= bc7_wide_block_limit(wide_max);
}

// deep: best error so far (4 B/block) + the winners of one family's two modes (2 x 16 B/block)
// wide: winners [5 modes][parts] x 16 B + candidates [18 slots] x (4 + 16) B per block
// a scan is split while that keeps all its waves resident at once (launch_bc7_wide): parts * blocks <= max(blocks, 262144)
static size_t wide_win_entries(size_t n) { return n > 262144 ? n : 262144; }
static size_t wide_workspace_bytes(size_t n)
{
    return (size_t)5 * wide_win_entries(n) * sizeof(uint4) + (((size_t)WIDE_SLOTS * n * sizeof(int32_t) + 15) & ~(size_t)15) + (size_t)WIDE_SLOTS * n * sizeof(uint4);
}
// fused shape, in 4-byte words from the start of the workspace (every region starts on a 16-byte boundary)
// a list of blocks for modes 1/3 with what its split scan and refinement need: block ids [cap], winners of the scan's shares [5 rows][cap]
// (rows 2, 3 used: list_scan_parts x listed <= cap), the listed blocks' texels [cap] x 64 B in list order
// pairs (bc7_pair_scan's header): per band the merged words [cap] x 2 x 8 B, the second list [cap], 64 shape buckets of cap / 8 listed slots and (behind the
// CTR_WORDS counters) PAIR_CTR_WORDS counters; each kind's two halves are contiguous, so a call without bands uses them as one
// rot tasks (bc7_rot_tasks' header): per band three rotation lists [3][cap] and their payload slots [3][cap] x 16 B, per block of the surface one merged
// word of 8 B: 68 B per block in all; each kind's two halves are contiguous again
struct ListRegion { size_t list, wins, compact, cap, pair_words, pair_redo, pair_buckets, pair_ctr, pair_cap, rot_lists, rot_payload; };
struct FusedLayout { size_t inc, list0, list1, list2, counts, words, rot_words; ListRegion band[2]; };
// Which regions a call's settings can touch (a `basic` call was sized like a `slow` one, 124 B per block instead of 36):
//   lists    the three block lists of the RGBA profiles' alpha-first order (and list13 of an RGB bounded call that runs as one band);
//   bands    the per-band lists and share winners of the bounded order (modes 1/3, mode 7 scanned over lists);
//   compact  the listed blocks' texels in list order (the RGB bounded order only);
//   pairs    the pair route's words, second lists and buckets (the RGB bounded order only, whatever ITW_BC7_PAIRS says);
//   rot      the rotation lists, merged words and payload slots of modes 4/5 (the same calls with three channels, whatever ITW_BC7_ROT_TASKS says).
struct FusedNeeds { bool lists, bands, compact, pairs, rot; };
static FusedNeeds fused_needs(const Bc7Modes& M)
{
    // (compact: sized with mode 7 on too, where no launch reads it)
    return FusedNeeds{M.alpha_first || M.bounded, M.bounded, M.bounded && !M.alpha_first && env_once(ENV_COMPACT), M.rgb_bounded, M.rgb_bounded && M.channels == 3};
}
static FusedLayout fused_layout(size_t n, const FusedNeeds& need)
{
    auto up4 = [](size_t w) { return (w + 3) & ~(size_t)3; };
    const size_t nchunks = (n + TPB - 1) / TPB;
    FusedLayout W;
    size_t o = up4(5 * n);                                         // 5 winner rows
    W.inc = o;      o = up4(o + n);                                // a phase's error / incumbent
    const size_t lcap = need.lists ? 2 * (nchunks / 2 + 65) * TPB : 0;   // three block lists (RGBA profiles), each with room for two bands' shares
    W.list0 = o;    o = up4(o + lcap);
    W.list1 = o;    o = up4(o + lcap);
    W.list2 = o;    o = up4(o + lcap);
    W.counts = o;   o += CTR_WORDS;                                // list lengths, the pilot's verdict
    for (int k = 0; k < 2; k++) { W.band[k].pair_ctr = o; o += PAIR_CTR_WORDS; }   // (contiguous with them: bc7_bounded_setup clears all of it)
    for (int k = 0; k < 2; k++) {                                  // the two bands: lists and share winners ...
        ListRegion& r = W.band[k];
        r.cap = (nchunks / 2 + 65) * TPB;                          // (a band is whole stripes of up to 64 chunks)
        r.list = o;    o = up4(o + (need.bands ? r.cap : 0));
        r.wins = o;    o = up4(o + (need.bands ? 5 * r.cap : 0));
    }
    W.band[0].compact = o; o += need.compact ? 16 * W.band[0].cap : 0;   // ... and their texels, contiguous: a call without bands uses both as one
    W.band[1].compact = o; o += need.compact ? 16 * W.band[1].cap : 0;
    for (int k = 0; k < 2; k++) { W.band[k].pair_words = o; o += need.pairs ? 4 * W.band[k].cap : 0; }
    for (int k = 0; k < 2; k++) { W.band[k].pair_redo = o; o += need.pairs ? W.band[k].cap : 0; }
    for (int k = 0; k < 2; k++) { W.band[k].pair_cap = W.band[k].cap / 8; W.band[k].pair_buckets = o; o += need.pairs ? 64 * W.band[k].pair_cap : 0; }
    W.rot_words = o; o = up4(o + (need.rot ? 2 * n : 0));
    for (int k = 0; k < 2; k++) { W.band[k].rot_lists = o; o += need.rot ? 3 * W.band[k].cap : 0; }
    for (int k = 0; k < 2; k++) { W.band[k].rot_payload = o; o += need.rot ? 12 * W.band[k].cap : 0; }
    W.words = o;
    return W;
}
bool bc7_scans_every_shape(const bc7_enc_settings& s) { return bc7_modes(s).bounded; }
// does a call with these settings run the bounded order of the RGB profiles (`slow`: the one order with a pilot)?  Only in the fused shape.
static bool has_order_verdict(const Bc7Modes& M) { return env_once(ENV_FUSED) && M.rgb_bounded; }
bool bc7_has_order_verdict(const bc7_enc_settings& s) { return has_order_verdict(bc7_modes(s)); }

size_t bc7_workspace_bytes(int width, int height, int64_t wide_max_blocks, const bc7_enc_settings* settings)
{
    const size_t n = (size_t)(width / 4) * (size_t)(height / 4);
    size_t deep = ((n * sizeof(int32_t) + 15) & ~(size_t)15) + 2 * n * sizeof(uint4);
    const FusedNeeds everything{true, true, true, true, true};                                  // unknown settings
    const size_t fused = fused_layout(n, settings ? fused_needs(bc7_modes(*settings)) : everything).words * sizeof(uint32_t);
    if (fused > deep) deep = fused;
    const bool may_wide = (int64_t)n <= bc7_wide_block_limit(wide_max_blocks);     // whatever the settings: they may change between sizing and launching
    const size_t wide = may_wide ? wide_workspace_bytes(n) : 0;
    return deep > wide ? deep : wide;
}

static void launch_bc7_wide(const Bc7Launch& L, const Bc7Modes& M, float* workspace, const Bc7Aux* aux)
{
    const uint8_t* src = L.src; const int64_t stride = L.stride, n = L.n; const int bx = L.bx; const bool vec = L.vec; hipStream_t st = L.st; const bc7_enc_settings& S = L.S;
    uint4* wins = reinterpret_cast<uint4*>(workspace);
    int32_t* cerr = reinterpret_cast<int32_t*>(wins + (size_t)5 * wide_win_entries((size_t)n));
    uint4* cblk = reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(cerr) + (((size_t)WIDE_SLOTS * n * sizeof(int32_t) + 15) & ~(size_t)15));
    const int ranked13 = M.r13, ranked7 = M.r7;
    const bool any_ranked = M.r13 || M.r7;

    // parts per scan: as many waves as stay resident at once (1024 SIMDs x the scan kernel's waves), within what the
    // candidate lists offer
    const int64_t waves = (n + 63) / 64;
    const int families = (M.on02 ? 1 : 0) + (M.on13 ? 1 : 0) + (M.on7 ? 1 : 0);
    const int resident = 1024 * (any_ranked ? 3 : WIDE_SCAN_WAVES);
    int want = 1;
    while (want < WIDE_MAX_PARTS && waves * families * want * WIDE_FILL_DIVISOR <= resident) want *= 2;
    auto cap = [&](int limit) { int p = want; while (p > limit) p /= 2; return p < 1 ? 1 : p; };
    auto parts_of_ranked = [](int len) { return len >= 8 ? 4 : len >= 2 ? 2 : 1; };    // a ranked share recomputes the 64 keys: few parts
    const int p02 = cap(16);                                                        // 16 or 64 shapes
    const int p13 = cap(M.r13 ? parts_of_ranked(M.len1 > M.len3 ? M.len1 : M.len3) : 16);
    const int p7 = cap(M.r7 ? parts_of_ranked(M.len7) : 16);
    auto larger = [](int a, int b) { return a > b ? a : b; };
    const int pstride = larger(larger(M.on02 ? p02 : 1, M.on13 ? p13 : 1), M.on7 ? p7 : 1);      // rows of the winners array per mode

    WideTasks T{};
    auto add = [&](int kind, int part, int parts) { T.kind[T.n] = (uint8_t)kind; T.part[T.n] = (uint8_t)part; T.parts[T.n] = (uint8_t)parts; T.n++; };
    WideModes R{}, G{};                                   // refine tasks (after the scans), single-subset tasks (independent)
    uint32_t active = 0;
    auto add_refine = [&](int mode, int parts) { R.mode[R.n] = (uint8_t)mode; R.parts[R.n] = (uint8_t)parts; R.n++; active |= 1u << wide_win_slot(mode); };
    auto add_single = [&](int code) { G.mode[G.n] = (uint8_t)code; G.parts[G.n] = 1; G.n++; };
    // longest tasks first: a launch drains in blockIdx order
    if (M.on13) { for (int p = 0; p < p13; p++) add(WK_SCAN13, p, p13); if (M.len1 > 0) add_refine(1, p13); if (M.len3 > 0) add_refine(3, p13); }
    if (M.on02) { for (int p = 0; p < p02; p++) add(WK_SCAN02, p, p02); add_refine(0, p02); if (!S.skip_mode2) add_refine(2, p02); }
    if (M.on7)  { for (int p = 0; p < p7; p++) add(WK_SCAN7, p, p7); add_refine(7, p7); }
    if (M.on45) {
        // one wave per rotation, or one per (rotation, candidate) while all those waves (2 per SIMD) stay resident at once
        const int rots = M.channels - S.mode45_channel0;
        const bool split = waves * (3 * rots + (M.on6 ? 1 : 0) + (aux ? 0 : R.n)) <= 2048;
        for (int r = S.mode45_channel0; r < M.channels; r++) {
            if (split) { for (int c = 0; c < 3; c++) add_single(100 + 4 * r + c); active |= 3u << (WIDE_SLOT_M4 + 2 * r); }
            else       { add_single(100 + 4 * r + 3); active |= 1u << (WIDE_SLOT_M4 + 2 * r); }
            active |= 1u << (WIDE_SLOT_M5 + r);
        }
    }
    if (M.on6)  { add_single(6); active |= 1u << WIDE_SLOT_M6; }

    const unsigned gx = (unsigned)((n + TPB - 1) / TPB);
    const dim3 blk(TPB);
    // the single-subset tasks need nothing from the scans: beside them on the caller-provided second stream, else after them
    hipStream_t gs = st;
    if (aux && G.n > 0 && T.n > 0) {
        (void)hipEventRecord(aux->fork, st);               // whatever feeds `src` on st (an upload) comes first
        (void)hipStreamWaitEvent(aux->stream, aux->fork, 0);
        gs = aux->stream;
    }
    auto phase2 = [&](auto singles, const WideModes& tasks, hipStream_t s) {
        with_bool(vec, [&](auto V) {
            hipLaunchKernelGGL((bc7_wide_phase2<decltype(V)::value, decltype(singles)::value>), dim3(gx, (unsigned)tasks.n), blk, 0, s, src, stride, bx, (int32_t)n, wins, cerr, cblk, S,
                               tasks, pstride);
        });
    };
    if (G.n > 0) {
        phase2(std::true_type{}, G, gs);
        if (gs != st) (void)hipEventRecord(aux->join, gs);
    }
    if (T.n > 0)
        with_bools(vec, any_ranked, [&](auto V, auto K) {
            hipLaunchKernelGGL((bc7_wide_phase1<decltype(V)::value, decltype(K)::value>), dim3(gx, (unsigned)T.n), blk, 0, st, src, stride, bx, (int32_t)n, wins, cerr, cblk, S, T,
                               ranked13, ranked7, pstride);
        });
    if (R.n > 0) phase2(std::false_type{}, R, st);
    if (gs != st) (void)hipStreamWaitEvent(st, aux->join, 0);
    hipLaunchKernelGGL(bc7_wide_commit, dim3(gx), blk, 0, st, cerr, cblk, (int32_t)n, active, reinterpret_cast<uint4*>(L.dst), vec ? 1 : 0);
}

// ---- the fused shape: a scan of all families and a refinement of all modes, in one of four mode orders -----------------------------------
// What launch_bc7 derives from the workspace for a fused call.
struct Fused {
    const Bc7Launch& L; const Bc7Modes& M; const Bc7Aux* aux; FusedLayout W; int32_t nchunks;
    uint32_t* wins4;         // [5 modes][n] x 4 B
    int32_t* alpha_err;      // [n] x 4 B behind the winner rows: a phase's error / incumbent
    int32_t* list_rgb;       // [n] block ids (RGBA profiles: where an RGB mode can win)
    int32_t* list13;         // [n] block ids (RGBA profiles, bounded order; RGB bounded order in one band: where modes 1/3 can win)
    int32_t* list7;          // [n] block ids (RGBA profiles, bounded order incl. mode 7)
    int32_t* ctr;            // the call's counter block (CTR_*), both bands' pair counters behind it
};
static Fused fused_context(const Bc7Launch& L, const Bc7Modes& M, float* workspace, const Bc7Aux* aux)
{
    Fused C{L, M, aux, fused_layout((size_t)L.n, fused_needs(M)), (int32_t)(((int64_t)L.n + TPB - 1) / TPB)};
    C.wins4 = reinterpret_cast<uint32_t*>(workspace);
    auto at = [&](size_t word) { return reinterpret_cast<int32_t*>(C.wins4 + word); };
    C.alpha_err = at(C.W.inc); C.list_rgb = at(C.W.list0); C.list13 = at(C.W.list1); C.list7 = at(C.W.list2); C.ctr = at(C.W.counts);
    return C;
}

// Where a launch runs.  `sel`: which chunks (ChunkSel); `cnt`: how many chunks that is (the grid); `s`: the stream; `wins`, `rows`: the winner rows it
// writes or reads and their length (n; a band's list scan has its own rows).
struct Span { ChunkSel sel; int32_t cnt; hipStream_t s; uint32_t* wins; int32_t rows; };
// A list of blocks to walk instead of the surface: ids, length, and (optional) the listed blocks' texels in list order.
struct BlockList { const int32_t* list; const int32_t* count; const uint4* compact; };
static const ChunkSel ALL_CHUNKS{0, 1, 0, nullptr, 0};
static const BlockList NO_LIST{nullptr, nullptr, nullptr};

// One band of a bounded order (the whole surface where the call runs as one): its chunks, its stream, the list of the blocks whose modes 1/3 a bound
// cannot exclude with the winner rows of that list's scan, and what the route adds -- the RGBA profiles' two other lists, or the RGB profiles' compact
// texels, pair route and rotation tasks.
struct Band {
    ChunkSel sel; int32_t cnt; hipStream_t s; int32_t* list; int32_t* count; uint32_t* wins; int32_t rows;
    int32_t* list_rgb; int32_t* count_rgb; int32_t* list7; int32_t* count7;            // alpha-first with mode 7 bounded
    uint4* compact; PairRegion P; int32_t* redo; RotRegion R;                          // RGB bounded
};
// the bounded orders run as two interleaved bands, one per stream, where the caller lends a second stream and the surface is large enough
static bool two_bands(const Fused& C) { return bc7_bands() > 1 && C.aux && !C.aux->single && C.aux->stream && C.nchunks >= 32; }
// The geometry both bounded routes share: stripes of 64 chunks (16 block rows of a 4096-wide surface), fewer on small surfaces; even stripes are band 0,
// odd stripes band 1.  A band's list scan has rows of its own: shares x listed blocks <= rows, so the scan's grid covers them (list_scan_parts).
static Band make_band(const Fused& C, bool two, int k, hipStream_t s)
{
    int32_t stripe = C.nchunks / 16;
    stripe = stripe < 1 ? 1 : (stripe > 64 ? 64 : stripe);
    const int32_t stripes = (C.nchunks + stripe - 1) / stripe;
    Band B{};
    B.sel = ChunkSel{two ? 1 : 0, stripe, k, nullptr, 0};
    B.cnt = two ? ((stripes + 1 - k) / 2) * stripe : C.nchunks;
    B.s = s;
    B.wins = two ? C.wins4 + C.W.band[k].wins : C.wins4;         // one band: the global winner rows
    B.rows = two ? B.cnt * TPB : C.L.n;
    return B;
}
static Span surface(const Fused& C) { return Span{ALL_CHUNKS, C.nchunks, C.L.st, C.wins4, C.L.n}; }
static Span band_chunks(const Fused& C, const Band& B) { return Span{B.sel, B.cnt, B.s, C.wins4, C.L.n}; }       // the band's chunks of the surface
static Span band_list(const Band& B) { return Span{ALL_CHUNKS, B.cnt, B.s, B.wins, B.rows}; }                   // a list of the band's, the band's own rows
static Span band_list_surface_rows(const Fused& C, const Band& B) { return Span{ALL_CHUNKS, B.cnt, B.s, C.wins4, C.L.n}; }

enum { SCAN02 = 1, SCAN13 = 2 };
// the {0,2} and / or {1,3} scan.  Interleave grain, measured at 4096^2 `slow` (scan time / scan FETCH_SIZE): 8 chunks 6.01 ms / 76 MB (two code paths
// alternate on every CU: instruction cache), 256 chunks 5.36 ms / 76 MB, 1024 chunks 5.38 ms / 166 MB (L2 no longer
// holds the first family's texels), family-major 5.39 ms / 154 MB; two separate launches 5.45 ms.
static void scan_rgb(const Fused& C, int families, const Span& sp, const BlockList& in = NO_LIST, int32_t split = 0)
{
    const Bc7Launch& L = C.L;
    ScanTasks T{};
    if (C.M.on13 && (families & SCAN13)) T.kind[T.n++] = WK_SCAN13;                   // longest first
    if (C.M.on02 && (families & SCAN02)) T.kind[T.n++] = WK_SCAN02;
    if (T.n == 0) return;
    const int32_t c8 = ((sp.cnt + 7) / 8) * 8;
    const int32_t grain = c8 < 256 ? c8 : 256;
    const int32_t groups = (c8 + grain - 1) / grain;
    const dim3 grid((unsigned)(groups * grain * T.n));
    with_bools(L.vec, C.M.r13, [&](auto V, auto K) {
        hipLaunchKernelGGL((bc7_scan_all<decltype(V)::value, decltype(K)::value, false>), grid, dim3(TPB), 0, sp.s, L.src, L.stride, L.bx, sp.rows, sp.wins, L.S, T,
                           C.M.r13 ? 1 : 0, C.M.r7 ? 1 : 0, sp.cnt, grain, in.list, in.count, split, sp.sel, in.compact);
    });
}
// the mode 7 scan: every chunk of the span, never a compact copy
static void scan_7(const Fused& C, const Span& sp, const BlockList& in = NO_LIST, int32_t split = 0)
{
    const Bc7Launch& L = C.L;
    if (!C.M.on7) return;
    const ScanTasks T7{1, {WK_SCAN7}};
    const int32_t chunks8 = ((sp.cnt + 7) / 8) * 8;
    with_bools(L.vec, C.M.r7, [&](auto V, auto K) {
        hipLaunchKernelGGL((bc7_scan_all<decltype(V)::value, decltype(K)::value, true>), dim3((unsigned)chunks8), dim3(TPB), 0, sp.s, L.src, L.stride, L.bx, sp.rows, sp.wins, L.S, T7,
                           C.M.r13 ? 1 : 0, C.M.r7 ? 1 : 0, sp.cnt, chunks8, in.list, in.count, split, ALL_CHUNKS, (const uint4*)nullptr);
    });
}
// What a finish phase reads and leaves besides the output blocks (bc7_finish_all's header says which phase uses what).
struct FinishIO {
    const int32_t* in_list = nullptr; const int32_t* in_count = nullptr; const uint4* in_compact = nullptr;
    int32_t* out_list = nullptr; int32_t* out_count = nullptr; uint4* out_compact = nullptr;
    int32_t* out_list7 = nullptr; int32_t* out_count7 = nullptr;
    RotRegion rot{nullptr, nullptr, nullptr, nullptr, 0};
    FinishIO& in(const int32_t* l, const int32_t* c, const uint4* texels = nullptr) { in_list = l; in_count = c; in_compact = texels; return *this; }
    FinishIO& out(int32_t* l, int32_t* c, uint4* texels = nullptr) { out_list = l; out_count = c; out_compact = texels; return *this; }
    FinishIO& out7(int32_t* l, int32_t* c) { out_list7 = l; out_count7 = c; return *this; }
    FinishIO& rotations(const RotRegion& r) { rot = r; return *this; }
};
// bounded_list_tail<true> reads its PairTarget at a fixed distance from the list length: only a band's own counter block will do
static bool band_list_length(const Fused& C, const int32_t* count)
{
    const int32_t* band0 = C.ctr + CTR_WORDS + PAIR_CTR_LIST;
    return count == band0 || count == band0 + PAIR_CTR_WORDS;
}
// a finish phase: list phases launch one workgroup per possible list chunk (they return at once behind the list's end)
template <int PH>
static void finish(const Fused& C, const Span& sp, const FinishIO& io = FinishIO())
{
    const Bc7Launch& L = C.L;
    if (PH == 3 && !band_list_length(C, io.out_count)) fail_msg("bc7_finish_all<3>: the list length must be word %d of a band's counter block", PAIR_CTR_LIST);
    with_bool(L.vec, [&](auto V) {
        hipLaunchKernelGGL((bc7_finish_all<decltype(V)::value, PH>), dim3((unsigned)sp.cnt), dim3(TPB), 0, sp.s, L.src, L.stride, L.bx, sp.rows, L.dst, sp.wins, L.S, C.alpha_err,
                           io.in_list, io.in_count, io.out_list, io.out_count, io.out_list7, io.out_count7, sp.sel, io.in_compact, io.out_compact, io.rot);
    });
}
// the tail behind finish<10>: the blocks of the span's chunks whose modes 1/3 a bound cannot exclude, from the incumbents finish<10> left
static void bound_list(const Fused& C, const Span& sp, const FinishIO& io)
{
    const Bc7Launch& L = C.L;
    if (!band_list_length(C, io.out_count)) fail_msg("bc7_bound_list: the list length must be word %d of a band's counter block", PAIR_CTR_LIST);
    with_bool(L.vec, [&](auto V) {
        hipLaunchKernelGGL((bc7_bound_list<decltype(V)::value>), dim3((unsigned)sp.cnt), dim3(TPB), 0, sp.s, L.src, L.stride, L.bx, sp.rows, (int32_t)L.S.channels,
                           (const int32_t*)C.alpha_err, io.out_list, io.out_count, sp.sel, io.out_compact);
    });
}

// Alpha-first with mode 7 bounded too: modes 4,5,6 | 0,2 first, then 1,3 and 7 each over its own list.  Round 5: seven dependent launches
// leave the chip partly empty seven times, so -- as for the RGB profiles below -- the surface is cut into two interleaved
// bands, each with its own lists and share winners, one per stream.
static void launch_alpha_first_bounded7(const Fused& C)
{
    const Bc7Aux* aux = C.aux;
    hipStream_t st = C.L.st;
    ITW_CHECK(hipMemsetAsync(C.ctr, 0, CTR_WORDS * sizeof(int32_t), st));  // the finish phases append to the lists through them
    const bool two = two_bands(C);
    if (two) ITW_ROUTE_SEEN(ITW_ROUTE_TWO_BANDS);
    auto chain = [&](int k, hipStream_t s) {
        Band B = make_band(C, two, k, s);
        const size_t share = two ? k * C.W.band[0].cap : 0;                 // a band's share of each list region
        int32_t* lengths = C.ctr + (k ? CTR_BAND1 : 0);
        B.list_rgb = C.list_rgb + share; B.count_rgb = lengths + CTR_LIST_RGB;
        B.list = C.list13 + share;       B.count = lengths + CTR_LIST_13;
        B.list7 = C.list7 + share;       B.count7 = lengths + CTR_LIST_7;
        const BlockList rgb{B.list_rgb, B.count_rgb, nullptr}, l13{B.list, B.count, nullptr}, l7{B.list7, B.count7, nullptr};
        finish<6>(C, band_chunks(C, B), FinishIO().out(B.list_rgb, B.count_rgb).out7(B.list7, B.count7));
        scan_rgb(C, SCAN02, band_list_surface_rows(C, B), rgb);
        finish<5>(C, band_list_surface_rows(C, B), FinishIO().in(B.list_rgb, B.count_rgb).out(B.list, B.count).out7(B.list7, B.count7));
        scan_rgb(C, SCAN13, band_list(B), l13, 1);
        finish<4>(C, band_list(B), FinishIO().in(B.list, B.count));
        scan_7(C, band_list(B), l7, 1);
        finish<7>(C, band_list(B), FinishIO().in(B.list7, B.count7));
    };
    if (!two) { chain(0, st); return; }
    ITW_CHECK(hipEventRecord(aux->fork, st));
    ITW_CHECK(hipStreamWaitEvent(aux->stream, aux->fork, 0));
    chain(1, aux->stream);
    chain(0, st);
    ITW_CHECK(hipEventRecord(aux->join, aux->stream));
    ITW_CHECK(hipStreamWaitEvent(st, aux->join, 0));
}

// Alpha-first: mode 7 scanned over the surface, modes 4,5,6,7 finished and the blocks where an RGB mode can still win listed; the RGB modes over that
// list -- bounded (modes 0,2, then 1,3 over what a bound leaves of it) or in one go.
static void launch_alpha_first(const Fused& C)
{
    ITW_CHECK(hipMemsetAsync(C.ctr, 0, CTR_WORDS * sizeof(int32_t), C.L.st));  // the finish phases append to the lists through them
    const Span all = surface(C);
    int32_t* count_rgb = C.ctr + CTR_LIST_RGB; int32_t* count13 = C.ctr + CTR_LIST_13;
    const BlockList rgb{C.list_rgb, count_rgb, nullptr}, l13{C.list13, count13, nullptr};
    scan_7(C, all);
    finish<1>(C, all, FinishIO().out(C.list_rgb, count_rgb));
    if (C.M.bounded) {
        scan_rgb(C, SCAN02, all, rgb);
        finish<5>(C, all, FinishIO().in(C.list_rgb, count_rgb).out(C.list13, count13));
        scan_rgb(C, SCAN13, all, l13, 1);
        finish<4>(C, all, FinishIO().in(C.list13, count13));
    } else {
        scan_rgb(C, SCAN02 | SCAN13, all, rgb);
        finish<2>(C, all, FinishIO().in(C.list_rgb, count_rgb));
    }
}

// ---- the RGB bounded order ------------------------------------------------------------------------------------------------------------
// RGB profiles whose modes 1/3 scan every shape (`slow`).  Round 4: scan {0,2} -> finish<3> (modes 0,2,4,5,6; lists the blocks
// whose modes 1/3 an exact bound cannot exclude) -> scan {1,3} over the list -> finish<4>.  Round 5, with a second stream:
//  * BANDS.  The surface is cut into two interleaved bands (stripes of chunks), one per stream: a band's four dependent
//    launches leave the chip partly empty at every boundary (a scan wave runs 0.6 ms), and the other band's work fills those
//    tails (5.23 -> 4.98 ms on the bench surface, 7.30 -> 7.00 on a photograph; four bands are slower again).
//  * PILOT.  The order pays where few blocks are listed and still costs a little where nearly all are (photographs: 94 %).
//    Behind band 0's {0,2} scan -- common to both orders -- bc7_pilot_estimate looks at 1/16 of the surface and leaves a
//    device word; BOTH continuations of each band are enqueued behind it, each gated on that word (ChunkSel.gate): the one
//    the pilot did not choose returns at once.  No host round trip, no block treated differently from its neighbours.
//    (A sample encoded ahead on a third stream was measured first: its chain of small launches could not get its share of a
//    chip the bands' scans fill, and the verdict arrived late: profiles/history/r05/r05d_bc7_pilot_timeline.txt.)
// `rot_tasks`: the rotation bound is the RGB profiles' (an RGBA profile's fill is alpha); a first rotation outside 0..3 keeps the inline walk
struct RgbRoute { bool two, pairs, rot_tasks, pilot; };

static Band rgb_band(const Fused& C, const RgbRoute& R, int k, hipStream_t s)
{
    const ListRegion& r = C.W.band[k];
    uint32_t* w = C.wins4;
    Band B = make_band(C, R.two, k, s);
    // one band: list13 of the call, and both bands' texels, buckets, rotation lists and payload slots as one region of twice the capacity
    B.list = R.two ? reinterpret_cast<int32_t*>(w + r.list) : C.list13;
    B.compact = env_once(ENV_COMPACT) ? reinterpret_cast<uint4*>(w + r.compact) : nullptr;
    B.P = PairRegion{reinterpret_cast<uint64_t*>(w + r.pair_words), reinterpret_cast<int32_t*>(w + r.pair_buckets), reinterpret_cast<int32_t*>(w + r.pair_ctr),
                     bc7_pair_cap((int32_t)(R.two ? r.pair_cap : 2 * r.pair_cap))};
    B.count = B.P.ctr + PAIR_CTR_LIST;
    B.redo = reinterpret_cast<int32_t*>(w + r.pair_redo);
    B.R = RotRegion{reinterpret_cast<int32_t*>(w + r.rot_lists), C.ctr + (k ? CTR_BAND1 : CTR_ROT), reinterpret_cast<unsigned long long*>(w + C.W.rot_words),
                    reinterpret_cast<uint4*>(w + r.rot_payload), (int32_t)(R.two ? r.cap : 2 * r.cap)};
    return B;
}
// the call's counters start at zero, each band's PairTarget behind its pair counters (one small launch where a memset was)
static void rgb_setup(const Fused& C, const RgbRoute& R, const Band& A, const Band& B)
{
    const PairTarget off{PairRegion{nullptr, nullptr, nullptr, 0}, nullptr};
    hipLaunchKernelGGL(bc7_bounded_setup, dim3(1), dim3(TPB), 0, C.L.st, C.ctr, R.pairs ? PairTarget{A.P, A.redo} : off, R.pairs ? PairTarget{B.P, B.redo} : off);
}
static void rgb_head(const Fused& C, const Band& B) { scan_rgb(C, SCAN02, band_chunks(C, B)); }
// the estimate behind band B's head scan; `host_counts` (optional): pinned host memory, for a host that reads the counts itself
static void rgb_pilot(const Fused& C, const Band& B, int32_t thr256, int32_t* host_counts)
{
    const Bc7Launch& L = C.L;
    with_bool(L.vec, [&](auto V) {
        hipLaunchKernelGGL((bc7_pilot_estimate<decltype(V)::value>), dim3((unsigned)((B.cnt + 7) / 8)), dim3(TPB), 0, L.st, L.src, L.stride, L.bx, L.n, C.wins4,
                           L.S.skip_mode2 ? 1 : 0, B.sel, C.ctr + CTR_PILOT, thr256, C.ctr + CTR_PILOT_FLAG, host_counts);
    });
}
// a band's two continuations behind its head scan: the bounded order (gated on the pilot's 1) and the reference's (gated on its 0)
static void rgb_tail(const Fused& C, const RgbRoute& R, const Band& B)
{
    const Bc7Launch& L = C.L;
    auto gated = [&](int32_t want) { Span g = band_chunks(C, B); if (R.pilot) { g.sel.gate = C.ctr + CTR_PILOT_FLAG; g.sel.want = want; } return g; };
    // pairs: finish<3> also leaves the (block, shape) pairs the bound cannot exclude, bucketed by shape (header above bc7_pair_scan)
    if (R.rot_tasks) {
        // modes 4/5 only for the (block, rotation) pairs a bound leaves (header above bc7_rot_tasks); empty lists where the pilot chose the other order
        finish<9>(C, gated(1), FinishIO().rotations(B.R));
        with_bool(L.vec, [&](auto V) { hipLaunchKernelGGL((bc7_rot_tasks<decltype(V)::value>), dim3((unsigned)B.cnt), dim3(TPB), 0, B.s, L.src, L.stride, L.bx, L.S, C.alpha_err, B.R); });
        finish<10>(C, gated(1), FinishIO().rotations(B.R));
        bound_list(C, gated(1), FinishIO().out(B.list, B.count, B.compact));
    } else
        finish<3>(C, gated(1), FinishIO().out(B.list, B.count, B.compact));
    if (R.pairs) {
        // the few blocks finish<8> defers take the full list scan behind it
        int32_t* redo_count = B.P.ctr + PAIR_CTR_REDO;
        const Span pair_words{ALL_CHUNKS, B.cnt, B.s, reinterpret_cast<uint32_t*>(B.P.words), B.rows};
        hipLaunchKernelGGL(bc7_pair_scan, dim3((unsigned)((B.cnt + 1) / 2)), dim3(TPB), 0, B.s, L.src, L.stride, L.bx, B.list, B.compact, L.S, B.P);
        finish<8>(C, pair_words, FinishIO().in(B.list, B.count, B.compact).out(B.redo, redo_count).out7(nullptr, B.P.ctr + PAIR_CTR_OVERFLOW));
        scan_rgb(C, SCAN13, band_list(B), BlockList{B.redo, redo_count, nullptr}, 1);
        finish<4>(C, band_list(B), FinishIO().in(B.redo, redo_count));
    } else {
        scan_rgb(C, SCAN13, band_list(B), BlockList{B.list, B.count, B.compact}, 1);    // an empty list (the other order): returns at once
        finish<4>(C, band_list(B), FinishIO().in(B.list, B.count, B.compact));
    }
    if (R.pilot) {
        scan_rgb(C, SCAN13, gated(0));
        finish<0>(C, gated(0));
    }
}
// ITW_BC7_PILOT_DEBUG=1: what the pilot, the rotation lists and the pair route counted in a two-band call (synchronises)
static void rgb_print_counters(const Fused& C, const RgbRoute& R, const Band& A, const Band& B)
{
    int32_t h[CTR_WORDS + 2 * PAIR_CTR_WORDS];
    ITW_CHECK(hipStreamSynchronize(C.L.st));
    ITW_CHECK(hipMemcpy(h, C.ctr, sizeof h, hipMemcpyDeviceToHost));
    const int32_t* p = h + CTR_PILOT; const int32_t* r0 = h + CTR_ROT; const int32_t* r1 = h + CTR_BAND1;
    std::fprintf(stderr, "bc7 pilot: estimate %d of %d sampled blocks listed -> %s; lists %d + %d of %lld blocks\n", p[PILOT_LISTED], p[PILOT_SAMPLED],
                 h[CTR_PILOT_FLAG] ? "bounded" : "reference order", h[CTR_WORDS + PAIR_CTR_LIST], h[CTR_WORDS + PAIR_CTR_WORDS + PAIR_CTR_LIST], (long long)C.L.n);
    if (R.rot_tasks) std::fprintf(stderr, "bc7 rot tasks: rotation lists %d / %d / %d (band 0) + %d / %d / %d (band 1)\n", r0[0], r0[1], r0[2], r1[0], r1[1], r1[2]);
    for (int k = 0; k < 2 && R.pairs; k++) {
        const PairRegion& P = (k ? B : A).P;
        int32_t c[PAIR_CTR_WORDS];
        ITW_CHECK(hipMemcpy(c, P.ctr, sizeof c, hipMemcpyDeviceToHost));
        long long sum = 0; int32_t top = 0;
        for (int i = 0; i < 64; i++) { sum += c[i]; top = c[i] > top ? c[i] : top; }
        std::fprintf(stderr, "bc7 pairs: band %d: %lld pairs, fullest bucket %d of %d, overflow %d, deferred to the full scan %d\n", k, sum, top, P.cap,
                     c[PAIR_CTR_OVERFLOW], c[PAIR_CTR_REDO]);
    }
}
// itwTestBc7CallCounters: the words ITW_BC7_PILOT_DEBUG prints, for a test to assert on (a call without bands: band 1's stay zero)
static void rgb_snapshot_counters(const Fused& C)
{
#ifdef ITW_TEST_HOOKS
    if (g_counters_armed.load(std::memory_order_relaxed)) {          // itwTestBc7CallCounters: the same words, for a test to assert on
        int32_t h[CTR_WORDS + 2 * PAIR_CTR_WORDS], out[ITW_BC7_CALL_COUNTERS] = {};
        ITW_CHECK(hipStreamSynchronize(C.L.st));
        ITW_CHECK(hipMemcpy(h, C.ctr, sizeof h, hipMemcpyDeviceToHost));
        out[ITW_BC7_CC_PILOT_LISTED] = h[CTR_PILOT + PILOT_LISTED]; out[ITW_BC7_CC_PILOT_SAMPLED] = h[CTR_PILOT + PILOT_SAMPLED]; out[ITW_BC7_CC_PILOT_FLAG] = h[CTR_PILOT_FLAG];
        for (int k = 0; k < 2; k++) {
            const int32_t* band = h + CTR_WORDS + k * PAIR_CTR_WORDS;
            for (int r = 0; r < 3; r++) out[ITW_BC7_CC_ROT_LISTS + 3 * k + r] = h[(k ? CTR_BAND1 : CTR_ROT) + r];
            out[ITW_BC7_CC_LISTED + k] = band[PAIR_CTR_LIST];
            for (int s = 0; s < 64; s++) out[ITW_BC7_CC_PAIRS + k] += band[s];
            out[ITW_BC7_CC_OVERFLOW + k] = band[PAIR_CTR_OVERFLOW];
            out[ITW_BC7_CC_REDO + k] = band[PAIR_CTR_REDO];
        }
        for (int i = 0; i < ITW_BC7_CALL_COUNTERS; i++) g_call_counters[i].store(out[i], std::memory_order_relaxed);
    }
#else
    (void)C;
#endif
}
static void launch_rgb_bounded(const Fused& C)
{
    const Bc7Aux* aux = C.aux;
    hipStream_t st = C.L.st;
    const bool two = two_bands(C), rotations_ok = C.M.channels == 3 && C.L.S.mode45_channel0 >= 0 && C.L.S.mode45_channel0 <= 3;
    const bool pairs = env_every_call(ENV_PAIRS), rot_tasks = env_every_call(ENV_ROT_TASKS) && rotations_ok;
    const RgbRoute R{two, pairs, rot_tasks, two && bc7_pilot_threshold() >= 0 && aux->mid};
    if (R.two) ITW_ROUTE_SEEN(ITW_ROUTE_TWO_BANDS);
    if (R.pilot) ITW_ROUTE_SEEN(ITW_ROUTE_PILOT);
    if (R.pairs) ITW_ROUTE_SEEN(ITW_ROUTE_PAIRS);
    if (R.rot_tasks) ITW_ROUTE_SEEN(ITW_ROUTE_ROT_TASKS);
    if (!R.two) {
        const Band B = rgb_band(C, R, 0, st);
        if (B.compact) ITW_ROUTE_SEEN(ITW_ROUTE_COMPACT);
        rgb_setup(C, R, B, B);
        // a staged run of a host-pointer call (abi.hip) wants the same estimate, left for the HOST to read under the next run's upload -- it picks
        // the launch shape of the remaining runs; a probe scans what the estimate looks at and nothing else
        const bool verdict = aux && aux->verdict && aux->verdict->event;
        const bool probe = verdict && aux->probe;
        if (verdict) ITW_ROUTE_SEEN(ITW_ROUTE_HOST_VERDICT);
        if (probe) ITW_ROUTE_SEEN(ITW_ROUTE_PROBE);
        if (probe) scan_rgb(C, SCAN02, Span{ChunkSel{2, 1, 0, nullptr, 0}, (C.nchunks + 7) / 8, st, C.wins4, C.L.n});
        else rgb_head(C, B);
        if (verdict) {
            rgb_pilot(C, B, 256, aux->verdict->host_counts_dev);
            ITW_CHECK(hipEventRecord(aux->verdict->event, st));
            aux->verdict->valid = true;
        }
        if (!probe) rgb_tail(C, R, B);
        rgb_snapshot_counters(C);
        return;
    }
    hipStream_t s2 = aux->stream;
    const Band A = rgb_band(C, R, 0, st), B = rgb_band(C, R, 1, s2);
    if (A.compact && B.compact) ITW_ROUTE_SEEN(ITW_ROUTE_COMPACT);
    rgb_setup(C, R, A, B);
    ITW_CHECK(hipEventRecord(aux->fork, st));                // whatever feeds `src` on st (an upload), and the setup above
    ITW_CHECK(hipStreamWaitEvent(s2, aux->fork, 0));
    rgb_head(C, B); rgb_head(C, A);
    if (R.pilot) {
        rgb_pilot(C, A, bc7_pilot_threshold(), nullptr);
        ITW_CHECK(hipEventRecord(aux->mid, st));
        ITW_CHECK(hipStreamWaitEvent(s2, aux->mid, 0));        // band 1's continuations start behind the verdict
    }
    rgb_tail(C, R, B); rgb_tail(C, R, A);
    ITW_CHECK(hipEventRecord(aux->join, s2));
    ITW_CHECK(hipStreamWaitEvent(st, aux->join, 0));
    if (env_once(ENV_PILOT_DEBUG)) rgb_print_counters(C, R, A, B);
    rgb_snapshot_counters(C);
}

// The reference's order in two launches: {0,2} and {1,3} scanned together, {7}, then every mode's refinement and {4,5}, {6}.
static void launch_reference_order(const Fused& C)
{
    scan_rgb(C, SCAN02 | SCAN13, surface(C));
    scan_7(C, surface(C));
    finish<0>(C, surface(C));
}

// A family at a time: a ranked list longer than 16 shapes keeps its keys in 64 KiB of LDS (RANKED == 1), or ITW_BC7_FUSED=0.
template <int FAMILY>
static void launch_ranked_family(Bc7Launch& L, bool ranked, bool long_list)
{
    if (!ranked) launch_search<FAMILY, 0>(L);
    else if (long_list) launch_search<FAMILY, 1>(L);
    else launch_search<FAMILY, 2>(L);
    launch_finish<FAMILY>(L);
}
static void launch_per_family(Bc7Launch& L, const Bc7Modes& M)
{
    if (M.on02) { launch_search<F_MODES02, 0>(L); launch_finish<F_MODES02>(L); }
    if (M.on13) launch_ranked_family<F_MODES13>(L, M.r13, M.long13);
    if (M.on7) launch_ranked_family<F_MODE7>(L, M.r7, M.long7);
    if (M.on45 || M.on6) launch_finish<F_MODES456>(L);
    if (L.first) ITW_CHECK(hipMemsetAsync(L.dst, 0, (size_t)L.n * 16, L.st));   // no mode enabled: defined (zero) output
}

// Families run in the reference's order (kernel.ispc:1970-1977): {0,2} -> {1,3} -> {7} -> {4,5} -> {6}, or in an order that gives the same bytes.
void launch_bc7(const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst,
                const bc7_enc_settings& s, float* workspace, hipStream_t st, const Bc7Aux* aux)
{
    const int bx = width / 4, by = height / 4;
    const int64_t n = (int64_t)bx * by;
    if (n <= 0) return;
    const Bc7Modes M = bc7_modes(s);
    Bc7Launch L;
    L.S = s;
    L.S.channels = M.channels;
    L.err = reinterpret_cast<int32_t*>(workspace);                // (the per-family kernels' layout)
    L.wins = reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(workspace) + (((size_t)n * sizeof(int32_t) + 15) & ~(size_t)15));
    L.vec = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    L.grid = dim3((unsigned)((n + TPB - 1) / TPB));
    L.st = st; L.src = src; L.stride = stride; L.bx = bx; L.n = (int32_t)n; L.dst = dst; L.first = 1;
    const bool single = aux && aux->single;
    if (aux && aux->probe && !has_order_verdict(M)) { ITW_ROUTE_SEEN(ITW_ROUTE_PROBE_IGNORED); return; }   // only the bounded order of the RGB profiles has a verdict to estimate
    if (!single && bc7_use_wide(n, L.S, M, aux ? aux->wide_max_blocks : 0)) { ITW_ROUTE_SEEN(ITW_ROUTE_WIDE); launch_bc7_wide(L, M, workspace, aux); return; }
    // two launches (scan of all families, refinement of all modes) unless a ranked list is longer than 16 shapes or ITW_BC7_FUSED=0
    if (!env_once(ENV_FUSED) || M.long13 || M.long7 || !M.any()) { ITW_ROUTE_SEEN(ITW_ROUTE_PER_FAMILY); launch_per_family(L, M); return; }
    const Fused C = fused_context(L, M, workspace, aux);
    if (M.alpha_first && M.bounded && M.on7 && !M.r7 && (M.on45 || M.on6)) { ITW_ROUTE_SEEN(ITW_ROUTE_ALPHA_FIRST_BOUNDED7); launch_alpha_first_bounded7(C); }
    else if (M.alpha_first) { ITW_ROUTE_SEEN(M.bounded ? ITW_ROUTE_ALPHA_FIRST_BOUNDED : ITW_ROUTE_ALPHA_FIRST_PLAIN); launch_alpha_first(C); }
    else if (M.rgb_bounded) { ITW_ROUTE_SEEN(ITW_ROUTE_RGB_BOUNDED); launch_rgb_bounded(C); }
    else { ITW_ROUTE_SEEN(ITW_ROUTE_REFERENCE_ORDER); launch_reference_order(C); }
}

} // namespace itw
