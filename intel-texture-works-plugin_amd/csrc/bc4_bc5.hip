// bc4_bc5.hip -- BC4 / BC5 encoders for gfx950, UNORM and SNORM.
//
// These two formats are the only ones the plugin does not send through kernel.ispc: IntelPlugin.cpp:271-273 hands the
// RGBA8 scratch image to DirectXTex (DirectX::Compress, TEX_COMPRESS_DEFAULT).  This file is the device replacement of
// that call: same block walk and partial-block rule (DirectXTexCompress.cpp:105-183), same endpoint optimiser
// (BC.h:727-856 OptimizeAlpha<false>, BC4BC5.cpp:186-238 FindEndPointsBC4U) and index choice (BC4BC5.cpp:314-337),
// evaluated in IEEE fp32 exactly as written, one rounding per operation (the library is built with -ffp-contract=off).
//
// Mapping: one lane per 8-byte channel block (BC5: lanes 2b and 2b+1 encode R and G of block b), so a wavefront writes
// 512 contiguous bytes; each lane keeps its 16 texel codes in 8 registers (two per dword) and runs the (at most eight)
// Newton iterations with a per-lane exit.
//
// Round 4 -- issue cycles, not instructions:
//   * FindClosestUNORM as RUN LENGTHS.  The reference searches 8 decoded levels per texel for the first strictly smallest
//     |level - texel| (16 x 8 x subtract / compare / two selects).  With 8-bit texels the function (red_0, red_1, v) -> index
//     has a domain of 256^3 cases, and for every endpoint pair it is piecewise constant in v with AT MOST 8 runs
//     (tests/test_bc45_index_table.py walks all 16.7 M cases against the reference's own FindClosestUNORM compiled from
//     BC4BC5.cpp; the pairs with red_0 == red_1, where the interpolated levels differ from the endpoints by an ulp, have at
//     most 5).  A kernel (bc45_build_index_table, once per device) runs the search AS WRITTEN for all 65 536 pairs and
//     stores, per pair, the 7 run starts and the 8 run indices (16 B; 1 MiB per device, L2 resident).  A block then loads ONE
//     entry and a texel's index is "how many run starts are <= v", looked up in the run-index word: two texels per dword,
//     add / and / add per run start on 2-cycle VOP2 forms, no float, no compare, no select.
//   * The Newton loop keeps a step's weights {c, d, c*c, d*d} (BC.h:729-732 quotients and their products: the same fp32
//     multiplications, done once) in one 16-byte LDS entry addressed by the step itself: the scale carries a factor 16
//     (exact: a power of two commutes with every rounding involved), so med3 / add / convert / and yield the entry's byte
//     offset.  Waves without a 6-step block (no texel 0 or 255 in 64 blocks) run a loop without the 6-step cases.
//   * Minimum / maximum of the 16 codes on packed halves (v_pk_min/max_u16: two texels per instruction), also for the 6-step
//     ramp's "smallest code above 0 / largest below 255" ((v + 255) & 255 and (v + 1) & 255 move the excluded code to the
//     other end of the range).
//
// SNORM (template argument SGN; D3DXEncodeBC4S/BC5S, BC4BC5.cpp:240-292, 339-362, 424-442, 515-546; OptimizeAlpha<true>): the same
// kernel over the texel codes BIASED by 128 (code ^ 0x80: signed order becomes unsigned order, so the packed minimum / maximum and the
// run table work unchanged).  A texel is max((float)code * (1/127), -1): codes -128 and -127 (biased 0 and 1) are both -1.0.  What
// differs is stated where it differs: the 6-step ramp's choice and start values, the loop's out-of-range sentinels, FloatToSNorm, the
// decoded levels, and an ESCAPE in the run table: 30 endpoint pairs, all with red_0 == red_1, have 12-19 runs (their interpolated levels
// sit an ulp apart, and the nearest one flips back and forth as the texel moves away).  Their entries carry the run count (> 8) and a
// lane that meets one runs FindClosestSNORM as written over its eight levels.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include <mutex>
#include <vector>
#include "kernels.hpp"
#include "host_rt.hpp"
#include "offset32_host.hpp"
#include "normal_prep.hpp"

namespace itw {
namespace {

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u16x2 as_u16x2(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ uint32_t as_u32(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b) { return as_u32(__builtin_elementwise_min(as_u16x2(a), as_u16x2(b))); }
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) { return as_u32(__builtin_elementwise_max(as_u16x2(a), as_u16x2(b))); }

constexpr float UNORM_SCALE = 1.0f / 255.0f;                     // XMLoadUByteN4's SSE path: integer * (1/255)
constexpr float SNORM_SCALE = 1.0f / 127.0f;                     // XMLoadByteN4's SSE path: integer * (1/127), then max with -1

// texel value of a code: UNORM code 0..255, SNORM the BIASED code (int8 code + 128)
template <bool SGN>
__device__ __forceinline__ float texel_of(float code)
{
    if (SGN) return fmaxf((code - 128.0f) * SNORM_SCALE, -1.0f);
    return code * UNORM_SCALE;
}

// ---- FindClosestUNORM, tabulated ---------------------------------------------------------------------------------------------
// BC4_UNORM::DecodeFromIndex (BC4BC5.cpp:50-72), as written
__device__ __forceinline__ void decoded_levels(float (&g)[8], uint32_t r0, uint32_t r1)
{
    const float f0 = (float)r0 / 255.0f, f1 = (float)r1 / 255.0f;
    g[0] = f0; g[1] = f1;
    const bool eight = r0 > r1;
#pragma unroll
    for (int k = 1; k <= 6; k++) {
        const float v8 = (f0 * (float)(7 - k) + f1 * (float)k) / 7.0f;
        const float v6 = (k <= 4) ? (f0 * (float)(5 - k) + f1 * (float)k) / 5.0f : (k == 5 ? 0.0f : 1.0f);
        g[k + 1] = eight ? v8 : v6;
    }
}

// BC4_SNORM::DecodeFromIndex (BC4BC5.cpp:106-131), as written; r0, r1 are the stored bytes
__device__ __forceinline__ void decoded_levels_snorm(float (&g)[8], uint32_t r0, uint32_t r1)
{
    const int b0 = (int)(int8_t)r0, b1 = (int)(int8_t)r1;
    const float f0 = (float)(b0 == -128 ? -127 : b0) / 127.0f, f1 = (float)(b1 == -128 ? -127 : b1) / 127.0f;
    g[0] = f0; g[1] = f1;
    const bool eight = b0 > b1;                                   // the raw bytes decide the form
#pragma unroll
    for (int k = 1; k <= 6; k++) {
        const float v8 = (f0 * (float)(7 - k) + f1 * (float)k) / 7.0f;
        const float v6 = (k <= 4) ? (f0 * (float)(5 - k) + f1 * (float)k) / 5.0f : (k == 5 ? -1.0f : 1.0f);
        g[k + 1] = eight ? v8 : v6;
    }
}

// FindClosestUNORM / FindClosestSNORM (BC4BC5.cpp:314-362): first index with the strictly smallest |g - t|
__device__ __forceinline__ uint32_t closest_level(const float (&g)[8], float t)
{
    uint32_t best = 0;
    float best_delta = 100000.0f;
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) {
        const float d = fabsf(g[k] - t);
        if (d < best_delta) { best = k; best_delta = d; }
    }
    return best;
}

// Entry of the run table for one endpoint pair: the index is constant on runs [T_j, T_j+1) of the texel code v, T_0 = 0.
//   x, y   C_j = 256 - T_j for run j = 1..7, one byte each (C_1 in the low byte of x; 0 = no such run): v + C_j carries into
//          bit 8 exactly when v >= T_j.  The top byte of y holds the number of runs (> 8 = the representation does not hold:
//          checked once after the build; SNORM: > 8 = the escape, allowed for red_0 == red_1 only).  SNORM: v is the biased code
//   z, w   index of run j in byte j (z: runs 0..3, w: runs 4..7): a v_perm_b32 with run counts as selector bytes looks up four
//          texels at once
template <bool SGN>
__global__ void __launch_bounds__(256) bc45_build_index_table(uint4* __restrict__ table)
{
    const uint32_t r0 = blockIdx.x, r1 = threadIdx.x;
    float g[8];
    if (SGN) decoded_levels_snorm(g, r0, r1);
    else     decoded_levels(g, r0, r1);
    uint32_t c[2] = {0u, 0u}, order[2] = {0u, 0u}, runs = 0u, prev = 8u;
    for (uint32_t v = 0; v < 256u; v++) {
        const uint32_t best = closest_level(g, texel_of<SGN>((float)v));
        if (best != prev) {
            if (runs >= 1u && runs < 8u) c[(runs - 1u) >> 2] |= (256u - v) << (8u * ((runs - 1u) & 3u));
            if (runs < 8u) order[runs >> 2] |= best << (8u * (runs & 3u));
            runs++;
            prev = best;
        }
    }
    table[r0 * 256u + r1] = make_uint4(c[0], c[1] | (min(runs, 255u) << 24), order[0], order[1]);
}

// ---- the normalise of a normal map, tabulated (itwCompressNormalMapBC5; normal_prep.hpp is the definition) -------------------------------
// NormalizeNormalMapChain scales a texel by s = 127.0f / sqrtf((r*r + g*g) + b*b), r, g, b = code - 128.  The three squares and their sums
// are integers below 2^24, so every fp32 operation up to the square root's argument is exact and s is a function of the INTEGER
// k = r^2 + g^2 + b^2 <= 3 * 128^2 alone: 49 153 floats, computed on the host (IEEE square root and divide) and kept right behind the UNORM
// run table, so the kernel needs no argument of its own.  Entry 0 is 0: the zero vector's R and G then come out as 0 * 0 + 128 = 128, the
// default normal's (its blue, 255, is not BC5's business).  One v_dot4_i32_i8 and one 4-byte read replace the square root and the divide.
constexpr uint32_t NORMAL_SCALE_ENTRIES = 3u * 128u * 128u + 1u;
constexpr size_t RUN_TABLE_BYTES = 65536 * sizeof(uint4);

struct TableSlot { std::once_flag once; uint4* table = nullptr; };
TableSlot g_tables[2][64];                                        // [0] UNORM, [1] SNORM: each built by the first call that needs it

// Built once per device on a stream of the library's own (not on the caller's -- the first call used to synchronise the user's
// stream): the first BC4 / BC5 call on a device, or itwWarmupBC45(), blocks its HOST thread until the table exists; the caller's stream is
// never synchronised and later calls are plain asynchronous launches.  That one call allocates device memory, so it cannot run inside a
// stream capture: warm up first (include/itw_bc45.h).
template <bool SGN>
const uint4* index_table()
{
    int dev = 0;
    ITW_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) fail_msg("BC4/BC5: device ordinal %d out of range", dev);
    TableSlot& s = g_tables[SGN ? 1 : 0][dev];
    std::call_once(s.once, [&] {                                  // an exception leaves the flag unset: the next call retries
        uint4* t = nullptr;
        hipStream_t own = nullptr;
        ITW_CHECK(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
        std::vector<float> scale(SGN ? 0u : NORMAL_SCALE_ENTRIES, 0.0f);        // the UNORM table carries the normalise scales behind its runs
        for (uint32_t k = 1; k < (uint32_t)scale.size(); k++) scale[k] = 127.0f / std::sqrt((float)k);
        hipError_t e = hipMalloc(&t, RUN_TABLE_BYTES + scale.size() * sizeof(float));
        if (e != hipSuccess) { (void)hipStreamDestroy(own); fail_hip("hipMalloc (BC4/BC5 index table)", e, __FILE__, __LINE__); }
        hipLaunchKernelGGL(bc45_build_index_table<SGN>, dim3(256), dim3(256), 0, own, t);
        std::vector<uint4> h(65536);
        e = hipMemcpyAsync(h.data(), t, 65536 * sizeof(uint4), hipMemcpyDeviceToHost, own);
        if (e == hipSuccess && !scale.empty()) e = hipMemcpyAsync(t + 65536, scale.data(), scale.size() * sizeof(float), hipMemcpyHostToDevice, own);
        if (e == hipSuccess) e = hipStreamSynchronize(own);       // complete before any later launch, on whatever stream
        (void)hipStreamDestroy(own);
        if (e != hipSuccess) { (void)hipFree(t); fail_hip("bc45_build_index_table", e, __FILE__, __LINE__); }
        for (size_t i = 0; i < h.size(); i++) {
            const uint32_t n = h[i].y >> 24;
            const bool escape_ok = SGN && (i >> 8) == (i & 255u);  // SNORM, red_0 == red_1: the lane searches the levels itself
            if (n < 1u || (n > 8u && !escape_ok)) { (void)hipFree(t); fail_msg("BC4/BC5 index table: an endpoint pair has %u runs (at most 8 expected)", n); }
        }
        s.table = t;
    });
    return s.table;
}

// ---- OptimizeAlpha<false> (BC.h:727-856) ---------------------------------------------------------------------------------------
// Step weights in LDS: entry s of table STEPS holds {c, d, c*c, d*d} with c = pC[s], d = pD[s] (BC.h:729-732: (STEPS-1-s)/(STEPS-1)
// and s/(STEPS-1) as compile-time fp32 quotients).  Entries 6 and 7 of the 6-step table are zero: the reference skips the codes
// "exactly 0" / "exactly 1" in its sums (`if (iStep < cSteps)`), and adding +-0 to an accumulator that started at +0 and only
// ever received sums of finite terms changes nothing (x + (+-0) = x; (+0) + (-0) = +0).
struct StepWeights { float c, d, cc, dd; };

__device__ __forceinline__ StepWeights step_weights(int steps, int s)
{
    // the quotients as the reference's tables hold them: k/7 and k/5 (k * (1/7) is not bit-equal to k/7 for k = 3 and 6)
    const float w8[8] = {0.0f / 7.0f, 1.0f / 7.0f, 2.0f / 7.0f, 3.0f / 7.0f, 4.0f / 7.0f, 5.0f / 7.0f, 6.0f / 7.0f, 7.0f / 7.0f};
    const float w6[6] = {0.0f / 5.0f, 1.0f / 5.0f, 2.0f / 5.0f, 3.0f / 5.0f, 4.0f / 5.0f, 5.0f / 5.0f};
    StepWeights r{0.f, 0.f, 0.f, 0.f};
    if (steps == 8)  { r.c = w8[7 - s]; r.d = w8[s]; }
    else if (s < 6)  { r.c = w6[5 - s]; r.d = w6[s]; }
    r.cc = r.c * r.c; r.dd = r.d * r.d;
    return r;
}

// One pass over the ramp for the lanes that are still iterating.  SIX = false: no lane of the wave has a 6-step block.
// `six` (per lane) selects the 6-step ramp; t[] are the texels as floats.
template <bool SIX, bool SGN>
__device__ __forceinline__ void newton_loop(float& fx, float& fy, const float (&t)[16], bool six, const StepWeights* tab8, const StepWeights* tab6)
{
    const float fsteps = (SIX && six) ? 5.0f : 7.0f;
    const float top16 = fsteps * 16.0f;
    const char* base = reinterpret_cast<const char*>((SIX && six) ? tab6 : tab8);
#pragma unroll 1
    for (int it = 0; it < 8; it++) {
        if ((fy - fx) < (1.0f / 256.0f)) break;
        const float scale = fsteps / (fy - fx);
        const float scale16 = scale * 16.0f;                      // exact: the step below comes out multiplied by 16 = its table offset
        // 6-step ramp: below the ramp the texel goes to "exactly 0" when it is nearer, above it to "exactly 1" (BC.h:789-804);
        // for 8-step lanes the two bounds are out of the texels' range ([0, 1], SNORM [-1, 1]).  SNORM keeps both rules as written
        // (BC.h:817, 819): they are not symmetric about 0
        const float to_zero = (SIX && six) ? fx * 0.5f : (SGN ? -2.0f : -1.0f);
        const float to_one  = (SIX && six) ? (fy + 1.0f) * 0.5f : 2.0f;
        float dx = 0.0f, dy = 0.0f, d2x = 0.0f, d2y = 0.0f;
        // four texels per batch: their steps first, then their four table reads in flight together, then the sums in texel order
        // (left to the compiler, every read was followed by its wait: sixteen serial LDS round trips per pass)
#pragma unroll
        for (int i0 = 0; i0 < 16; i0 += 4) {
            uint32_t off[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = i0 + u;
                const float dot16 = (t[i] - fx) * scale16;
                // dot <= 0 -> step 0, dot >= fsteps -> the last step, else (int)(dot + 0.5): clamp first, the clamped ends convert to themselves
                const float m = __builtin_amdgcn_fmed3f(dot16, 0.0f, top16);
                off[u] = (uint32_t)(int32_t)(m + 8.0f) & 0x70u;
                if (SIX) {
                    if (dot16 <= 0.0f && t[i] <= to_zero) off[u] = 6u * 16u;
                    if (dot16 >= top16 && t[i] >= to_one) off[u] = 7u * 16u;
                }
            }
            StepWeights w[4];
#pragma unroll
            for (int u = 0; u < 4; u++) w[u] = *reinterpret_cast<const StepWeights*>(base + off[u]);
            __builtin_amdgcn_sched_barrier(0);                    // keep the four reads ahead of the arithmetic that consumes them
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const float diff = (w[u].c * fx + w[u].d * fy) - t[i0 + u];
                dx += w[u].c * diff;
                d2x += w[u].cc;
                dy += w[u].d * diff;
                d2y += w[u].dd;
            }
        }
        if (d2x > 0.0f) fx -= dx / d2x;
        if (d2y > 0.0f) fy -= dy / d2y;
        if (fx > fy) { const float f = fx; fx = fy; fy = f; }
        if ((dx * dx < (1.0f / 64.0f)) && (dy * dy < (1.0f / 64.0f))) break;
    }
}

// One channel of one block -> 8 bytes (D3DXEncodeBC4U, BC4BC5.cpp:403-421).  P[j] = code of texel 2j | code of texel 2j+1 << 16.
__device__ __forceinline__ uint2 encode_channel(const uint32_t (&P)[8], const StepWeights* tab8, const StepWeights* tab6, const uint4* __restrict__ runs)
{
    float t[16];
#pragma unroll
    for (int j = 0; j < 8; j++) {                                 // one v_cvt_f32_ubyteN per texel, straight from the packed pair
        float lo, hi;
        asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(lo) : "v"(P[j]));
        asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(hi) : "v"(P[j]));
        t[2 * j] = lo * UNORM_SCALE;
        t[2 * j + 1] = hi * UNORM_SCALE;
    }
    // smallest / largest code, and for the 6-step ramp the smallest above 0 / largest below 255 (BC.h:742-766; fX starts at
    // 1.0 = code 255 and fY at 0.0 = code 0, which is also what "no such texel" leaves behind)
    uint32_t mn = P[0], mx = P[0];
#pragma unroll
    for (int j = 1; j < 8; j++) { mn = pk_min_u16(mn, P[j]); mx = pk_max_u16(mx, P[j]); }
    const uint32_t cmin = min(mn & 0xffffu, mn >> 16), cmax = max(mx & 0xffffu, mx >> 16);
    const bool six = (cmin == 0u) || (cmax == 255u);                     // BC4BC5.cpp:213: 0.0f == fBlockMin || 1.0f == fBlockMax
    const bool any_six = __any(six);                                     // wave-uniform: most waves have no 6-step block at all
    uint32_t cx = cmin, cy = cmax;
    if (any_six) {
        uint32_t lo6 = (P[0] + 0x00ff00ffu) & 0x00ff00ffu, hi6 = (P[0] + 0x00010001u) & 0x00ff00ffu;
#pragma unroll
        for (int j = 1; j < 8; j++) {
            lo6 = pk_min_u16(lo6, (P[j] + 0x00ff00ffu) & 0x00ff00ffu);   // (v - 1) mod 256: code 0 becomes the largest
            hi6 = pk_max_u16(hi6, (P[j] + 0x00010001u) & 0x00ff00ffu);   // (v + 1) mod 256: code 255 becomes the smallest
        }
        if (six) {
            const uint32_t l = min(lo6 & 0xffffu, lo6 >> 16), h = max(hi6 & 0xffffu, hi6 >> 16);
            cx = min(l + 1u, 255u);
            cy = h ? h - 1u : 0u;
        }
    }
    float fx = (float)cx * UNORM_SCALE, fy = (float)cy * UNORM_SCALE;
    if (six && fx == fy) fy = 1.0f;
    if (any_six) newton_loop<true, false>(fx, fy, t, six, tab8, tab6);
    else            newton_loop<false, false>(fx, fy, t, false, tab8, tab6);
    const float ox = (fx < 0.0f) ? 0.0f : (fx > 1.0f) ? 1.0f : fx;
    const float oy = (fy < 0.0f) ? 0.0f : (fy > 1.0f) ? 1.0f : fy;
    // BC4BC5.cpp:213-237: the 8-step ramp stores (max, min), the 6-step ramp (min, max)
    const uint32_t qx = (uint32_t)(ox * 255.0f), qy = (uint32_t)(oy * 255.0f);
    const uint32_t r0 = six ? qx : qy, r1 = six ? qy : qx;

    // FindClosestUNORM through the run table: count the run starts that are <= v, two texels per dword
    const uint4 e = runs[(r0 << 8) | r1];
    uint32_t C[7];
#pragma unroll
    for (int j = 0; j < 7; j++)
        C[j] = __builtin_amdgcn_perm(0u, j < 4 ? e.x : e.y, 0x0c000c00u | (uint32_t)((j & 3) * 0x00010001));   // byte j -> both halves
    // run indices as bytes (e.z: runs 0..3, e.w: runs 4..7): a v_perm_b32 whose selector bytes are the run counts (0..7) of FOUR
    // texels looks all four up at once
    const uint32_t tab_lo = e.z, tab_hi = e.w;
    const uint32_t carry = 0x01000100u;
    uint32_t part[2] = {0u, 0u};                                  // 3-bit indices of texels 0..7 / 8..15
#pragma unroll
    for (int q = 3; q >= 0; q--) {                                // four texels (two pairs) per step, from the last down: (acc << 12) | 12 bits
        uint32_t sa = (P[2 * q] + C[0]) & carry, sb = (P[2 * q + 1] + C[0]) & carry;
#pragma unroll
        for (int k = 1; k < 7; k++) { sa += (P[2 * q] + C[k]) & carry; sb += (P[2 * q + 1] + C[k]) & carry; }
        // the counts sit in bytes 1 and 3 of each sum: gather them in texel order, look the run indices up, squeeze 4 x 3 bits together
        const uint32_t counts = __builtin_amdgcn_perm(sb, sa, 0x07050301u);
        const uint32_t idx = __builtin_amdgcn_perm(tab_hi, tab_lo, counts);
        const uint32_t two = (idx | (idx >> 5)) & 0x003f003fu;    // texels (0,1) in bits 0..5, (2,3) in bits 16..21
        const uint32_t four = (two | (two >> 10)) & 0x0fffu;
        uint32_t& acc = part[q >> 1];
        acc = (acc << 12) | four;
    }
    return make_uint2(r0 | (r1 << 8) | (part[0] << 16), (part[0] >> 16) | (part[1] << 8));
}

// ---- the SNORM encoders (D3DXEncodeBC4S; the UNORM function above is kept as it was, instruction for instruction) ---------------------------
// FindClosestSNORM through the run table: the sixteen 3-bit indices of the biased codes in P for the stored endpoint bytes r0, r1; texels
// 0..7 in the low 24 bits of part[0], 8..15 in part[1].  The encoders and the test hook (itwTestBc45ClosestS) share it.
__device__ __forceinline__ void closest_indices_snorm(uint32_t (&part)[2], const uint32_t (&P)[8], uint32_t r0, uint32_t r1, const uint4* __restrict__ runs)
{
    // count the run starts that are <= v, two texels per dword
    const uint4 e = runs[(r0 << 8) | r1];
    uint32_t C[7];
#pragma unroll
    for (int j = 0; j < 7; j++)
        C[j] = __builtin_amdgcn_perm(0u, j < 4 ? e.x : e.y, 0x0c000c00u | (uint32_t)((j & 3) * 0x00010001));   // byte j -> both halves
    // run indices as bytes (e.z: runs 0..3, e.w: runs 4..7): a v_perm_b32 whose selector bytes are the run counts (0..7) of FOUR
    // texels looks all four up at once
    const uint32_t tab_lo = e.z, tab_hi = e.w;
    const uint32_t carry = 0x01000100u;
    part[0] = 0u; part[1] = 0u;                                   // 3-bit indices of texels 0..7 / 8..15
#pragma unroll
    for (int q = 3; q >= 0; q--) {                                // four texels (two pairs) per step, from the last down: (acc << 12) | 12 bits
        uint32_t sa = (P[2 * q] + C[0]) & carry, sb = (P[2 * q + 1] + C[0]) & carry;
#pragma unroll
        for (int k = 1; k < 7; k++) { sa += (P[2 * q] + C[k]) & carry; sb += (P[2 * q + 1] + C[k]) & carry; }
        // the counts sit in bytes 1 and 3 of each sum: gather them in texel order, look the run indices up, squeeze 4 x 3 bits together
        const uint32_t counts = __builtin_amdgcn_perm(sb, sa, 0x07050301u);
        const uint32_t idx = __builtin_amdgcn_perm(tab_hi, tab_lo, counts);
        const uint32_t two = (idx | (idx >> 5)) & 0x003f003fu;    // texels (0,1) in bits 0..5, (2,3) in bits 16..21
        const uint32_t four = (two | (two >> 10)) & 0x0fffu;
        uint32_t& acc = part[q >> 1];
        acc = (acc << 12) | four;
    }
    // the escape: an entry with more than 8 runs (30 pairs, all red_0 == red_1) does not describe its pair; such a lane searches the
    // eight decoded levels as written.  Rare (a wave skips it unless one of its 64 blocks landed on such a pair).
    const bool escape = (e.y >> 24) > 8u;
    if (__any(escape)) {
        if (escape) {
            float g[8];
            decoded_levels_snorm(g, r0, r1);
            part[0] = 0u; part[1] = 0u;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint32_t lo = closest_level(g, texel_of<true>((float)(P[j] & 0xffu)));
                const uint32_t hi = closest_level(g, texel_of<true>((float)(P[j] >> 16)));
                part[j >> 2] |= (lo | (hi << 3)) << (6 * (j & 3));
            }
        }
    }
}

// One channel of one block -> 8 bytes (D3DXEncodeBC4S, BC4BC5.cpp:424-442).  P[j] = biased code of texel 2j | biased code of texel 2j+1 << 16,
// every code >= 1.
__device__ __forceinline__ uint2 encode_channel_snorm(const uint32_t (&P)[8], const StepWeights* tab8, const StepWeights* tab6, const uint4* __restrict__ runs)
{
    // The kernel hands over biased codes >= 1: int8 -128 was read as -127 on packed halves as the codes were gathered (both are -1.0f, and
    // -127 * (1/127) is exactly -1.0f), so the texel is the sign-extended byte times 1/127 with no clamp left to do.
    float t[16];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t R = P[j] ^ 0x00800080u;                    // back to two's complement
        t[2 * j] = (float)(int32_t)(int8_t)(R & 0xffu) * SNORM_SCALE;
        t[2 * j + 1] = (float)(int32_t)(int8_t)((R >> 16) & 0xffu) * SNORM_SCALE;
    }
    // smallest / largest code, and for the 6-step ramp the smallest texel above -1.0 / largest below 1.0 (BC.h:742-766; fX starts at
    // 1.0 = biased code 255 and fY at -1.0, which is also what "no such texel" leaves behind).  -1.0 is biased code 0 AND code 1 (int8 -128
    // and -127): the ramp is chosen by "smallest <= 1 or largest == 255", fX is the smallest code above 1, and fY's start, -1.0, is what
    // codes 0 and 1 both convert to.
    uint32_t mn = P[0], mx = P[0];
#pragma unroll
    for (int j = 1; j < 8; j++) { mn = pk_min_u16(mn, P[j]); mx = pk_max_u16(mx, P[j]); }
    const uint32_t cmin = min(mn & 0xffffu, mn >> 16), cmax = max(mx & 0xffffu, mx >> 16);
    const bool six = (cmin <= 1u) || (cmax == 255u);                     // BC4BC5.cpp:267: -1.0f == fBlockMin || 1.0f == fBlockMax
    const bool any_six = __any(six);                                     // wave-uniform: most waves have no 6-step block at all
    uint32_t cx = cmin, cy = cmax;
    if (any_six) {
        constexpr uint32_t DOWN = 0x00fe00feu;                           // (v - 2) mod 256: the two excluded low codes become the largest
        uint32_t lo6 = (P[0] + DOWN) & 0x00ff00ffu, hi6 = (P[0] + 0x00010001u) & 0x00ff00ffu;
#pragma unroll
        for (int j = 1; j < 8; j++) {
            lo6 = pk_min_u16(lo6, (P[j] + DOWN) & 0x00ff00ffu);
            hi6 = pk_max_u16(hi6, (P[j] + 0x00010001u) & 0x00ff00ffu);   // (v + 1) mod 256: code 255 becomes the smallest
        }
        if (six) {
            const uint32_t l = min(lo6 & 0xffffu, lo6 >> 16), h = max(hi6 & 0xffffu, hi6 >> 16);
            cx = min(l + 2u, 255u);
            cy = h ? h - 1u : 0u;
        }
    }
    float fx = texel_of<true>((float)cx), fy = texel_of<true>((float)cy);
    if (six && fx == fy) fy = 1.0f;
    if (any_six) newton_loop<true, true>(fx, fy, t, six, tab8, tab6);
    else            newton_loop<false, true>(fx, fy, t, false, tab8, tab6);
    const float ox = (fx < -1.0f) ? -1.0f : (fx > 1.0f) ? 1.0f : fx;
    const float oy = (fy < -1.0f) ? -1.0f : (fy > 1.0f) ? 1.0f : fy;
    // FloatToSNorm (BC4BC5.cpp:161-182): NaN -> 0, clamp (a second time), * 127, +-0.5 by sign, truncate: never -128
    auto snorm = [](float f) -> uint32_t {
        if (f != f) f = 0.0f;
        else if (f > 1.0f) f = 1.0f;
        else if (f < -1.0f) f = -1.0f;
        f = f * 127.0f;
        f = (f >= 0.0f) ? f + 0.5f : f - 0.5f;
        return (uint32_t)(int32_t)f & 0xffu;
    };
    const uint32_t qx = snorm(ox), qy = snorm(oy);
    // BC4BC5.cpp:267-291: the 8-step ramp stores (max, min), the 6-step ramp (min, max)
    const uint32_t r0 = six ? qx : qy, r1 = six ? qy : qx;

    uint32_t part[2];
    closest_indices_snorm(part, P, r0, r1, runs);
    return make_uint2(r0 | (r1 << 8) | (part[0] << 16), (part[0] >> 16) | (part[1] << 8));
}

// register budget (waves per SIMD) and grid, tuning constants like the BC7 kernels'
#ifndef BC45_WAVES
#define BC45_WAVES 4
#endif
#ifndef BC45_GRID
#define BC45_GRID 2048
#endif

// The sixteen texel words of channel-block `lane` (4 x dwordx4 when VEC16 and the block is whole).  Partial blocks: missing columns /
// rows repeat source column / row {0,0,0,1}[i], itself wrapped to 0 when that one is missing too (bc45_fill_index, kernels.hpp).
template <int NCH, bool VEC16>
__device__ __forceinline__ void load_words45(uint32_t (&w)[16], const uint8_t* __restrict__ src, int64_t stride, int32_t width, int32_t height,
                                             int32_t blocks_x, int32_t lane)
{
    const int32_t b = (NCH == 2) ? (lane >> 1) : lane;
    const int32_t yy = b / blocks_x, xx = b - yy * blocks_x;
    const int32_t pw = min(4, width - 4 * xx), ph = min(4, height - 4 * yy);
    const uint8_t* p = src + (int64_t)yy * 4 * stride + (int64_t)xx * 16;
    if (pw == 4 && ph == 4) {
#pragma unroll
        for (int y = 0; y < 4; y++) {
            if (VEC16) {
                const uint4 v = *reinterpret_cast<const uint4*>(p + y * stride);
                w[4 * y] = v.x; w[4 * y + 1] = v.y; w[4 * y + 2] = v.z; w[4 * y + 3] = v.w;
            } else {
                const uint32_t* q = reinterpret_cast<const uint32_t*>(p + y * stride);
                w[4 * y] = q[0]; w[4 * y + 1] = q[1]; w[4 * y + 2] = q[2]; w[4 * y + 3] = q[3];
            }
        }
    } else {
#pragma unroll
        for (int y = 0; y < 4; y++) {
            const int sy = bc45_fill_index(y, ph);
#pragma unroll
            for (int x = 0; x < 4; x++) {
                const int sx = bc45_fill_index(x, pw);
                w[4 * y + x] = *reinterpret_cast<const uint32_t*>(p + sy * stride + sx * 4);
            }
        }
    }
}

// The packed codes of channel `ch` (0 = R, 1 = G) of sixteen NORMALISED texels (PREP has ITW_NORMAL_NORMALIZE; its flip bits apply first):
// what the v_perm gather yields for a surface prepared by normal_prep_rgba8.  Per texel: the three signed bytes code - 128 (the code with its
// top bit flipped), their sum of squares by one v_dot4_i32_i8, the scale from the table, and this lane's channel alone as
// (uint32_t)(x * s + 128.0f) -- both lanes of a block read the same sixteen scales, neither computes a square root or a divide.
template <uint32_t PREP>
__device__ __forceinline__ void normalised_codes(uint32_t (&P)[8], const uint32_t (&w)[16], uint32_t ch, const float* __restrict__ scale)
{
    constexpr uint32_t flip = ((PREP & 1u) ? 0x000000ffu : 0u) | ((PREP & 2u) ? 0x0000ff00u : 0u);
    uint32_t a[16];
    float s[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        a[i] = (w[i] ^ (flip ^ 0x00808080u)) & 0x00ffffffu;       // alpha out of the dot product
        s[i] = scale[__builtin_amdgcn_sdot4((int)a[i], (int)a[i], 0, false)];
    }
    const uint32_t up = 24u - 8u * ch;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const float x0 = (float)((int32_t)(a[2 * j] << up) >> 24), x1 = (float)((int32_t)(a[2 * j + 1] << up) >> 24);
        P[j] = (uint32_t)(x0 * s[2 * j] + 128.0f) | ((uint32_t)(x1 * s[2 * j + 1] + 128.0f) << 16);
    }
}

// ---- signed normal sources in the BC5_SNORM load (itwCompressNormalMapBC5S; normal_prep.hpp is the definition) ---------------------------
// A block of a TB-byte source is 16 * TB bytes (RGBA16F 128, RGBA32F 256), so the two lanes of a block do not each load all of it: lane
// `half` (0: the R lane, 1: the G lane) loads texel rows 2 * half and 2 * half + 1 -- with halfs the sixteen words the RGBA8 kernels
// prefetch -- runs the definition on its eight texels (eight square roots and divides, not sixteen), and hands the neighbour the four
// packed dwords of the channel the neighbour encodes.  Of a float texel only x, y, z are kept (alpha is not BC5's business): 24 words.
template <int TB> constexpr int kept_words() { return TB == 16 ? 3 : TB / 4; }

// four consecutive texels of one row at p into wr[0 .. 4 * kept_words)
template <int TB, bool VEC16>
__device__ __forceinline__ void load_row45(uint32_t* wr, const uint8_t* p)
{
    if (TB == 16) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(VEC16 ? __builtin_assume_aligned(p, 16) : p);
#pragma unroll
        for (int x = 0; x < 4; x++) { wr[3 * x] = q[4 * x]; wr[3 * x + 1] = q[4 * x + 1]; wr[3 * x + 2] = q[4 * x + 2]; }
    } else if (VEC16) {
#pragma unroll
        for (int k = 0; k < TB / 4; k++) { const uint4 v = reinterpret_cast<const uint4*>(p)[k]; wr[4 * k] = v.x; wr[4 * k + 1] = v.y; wr[4 * k + 2] = v.z; wr[4 * k + 3] = v.w; }
    } else {
#pragma unroll
        for (int k = 0; k < TB; k++) wr[k] = reinterpret_cast<const uint32_t*>(p)[k];
    }
}

// The eight texels of rows 2 * half, 2 * half + 1 of block `b`, any block: partial ones by bc45_fill_index, texel by texel
template <int TB, bool VEC16>
__device__ __forceinline__ void load_rows45(uint32_t (&w)[8 * kept_words<TB>()], const uint8_t* __restrict__ src, int64_t stride, int32_t width, int32_t height,
                                            int32_t blocks_x, int32_t b, int32_t half)
{
    constexpr int KW = kept_words<TB>();
    const int32_t yy = b / blocks_x, xx = b - yy * blocks_x;
    const int32_t pw = min(4, width - 4 * xx), ph = min(4, height - 4 * yy);
    const uint8_t* p = src + (int64_t)yy * 4 * stride + (int64_t)xx * 4 * TB;
    if (pw == 4 && ph == 4) {
#pragma unroll
        for (int r = 0; r < 2; r++) load_row45<TB, VEC16>(&w[4 * KW * r], p + (int64_t)(2 * half + r) * stride);
    } else {
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int sy = bc45_fill_index(2 * half + r, ph);
#pragma unroll
            for (int x = 0; x < 4; x++) {
                const uint32_t* q = reinterpret_cast<const uint32_t*>(p + (int64_t)sy * stride + bc45_fill_index(x, pw) * TB);
#pragma unroll
                for (int k = 0; k < KW; k++) w[(4 * r + x) * KW + k] = q[k];
            }
        }
    }
}

// The lane's eight texels through the definition: `own` = the biased codes (int8 code + 128, never below 1) of the channel this lane encodes
// (ch 0: x, 1: y), packed two per dword as encode_channel_snorm takes them, `send` = the other channel's, for the neighbour
template <int TB>
__device__ __forceinline__ void signed_normal_codes(uint32_t (&own)[4], uint32_t (&send)[4], const uint32_t (&w)[8 * kept_words<TB>()], uint32_t ch, uint32_t ops)
{
    constexpr int KW = kept_words<TB>();
#pragma unroll
    for (int j = 0; j < 4; j++) {
        uint32_t c[2][2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const uint32_t* t = &w[(2 * j + u) * KW];
            float v[4];
            if (TB == 16) normal_load_rgba32f(v, t[0], t[1], t[2], 0u);
            else          normal_load_signed<TB>(v, t);
            normal_signed_ops(v, ops);
            c[u][0] = (uint32_t)(normal_quantize_snorm(v[0]) + 128);
            c[u][1] = (uint32_t)(normal_quantize_snorm(v[1]) + 128);
        }
        const uint32_t x = c[0][0] | (c[1][0] << 16), y = c[0][1] | (c[1][1] << 16);
        own[j] = ch ? y : x;
        send[j] = ch ? x : y;
    }
}

// waves per SIMD of an instantiation: a whole-block float source keeps 24 prefetched words in flight where the others keep 16 or 8, which the
// 128 registers of four waves do not hold without scratch (16 B spilled); it alone is budgeted for three waves of 168 and takes 139
constexpr int bc45_waves(uint32_t prep, bool whole) { return (prep == 256u && whole) ? 3 : BC45_WAVES; }

// Persistent workgroups (round 4): a wave of this kernel executes ~630 VALU instructions per block -- a fifth of it waiting for its
// own texels if it loads, encodes, stores and exits (measured: 55-62 % of the issue slots used).  So at most BC45_GRID workgroups walk
// the surface in chunks of 256 channel blocks and request the NEXT chunk's texels before encoding the current one.
// WHOLE (the common case: width and height multiples of 4, the surface below 2 GiB): no partial blocks, and the walk keeps each
// lane's block position and byte offset incrementally -- one division per workgroup instead of one per chunk, 32-bit offsets from the
// uniform base instead of four 64-bit row pointers with their source-row / column selects (about 90 of the 630 instructions).
// SGN (trailing, so that the UNORM instantiations keep their names): the SNORM encoders; the texel codes are biased as they are gathered.
// PREP (trailing likewise; BC5_UNORM only): the normal-map stages ITW_NORMAL_* of normal_prep.hpp applied to the sixteen loaded words as
// their codes are gathered -- at the top of the loop, so the texels of the first load and of every prefetch take the same path.  A flip is
// an exclusive-or of the gathered codes; the normalise is normalised_codes above, its scale table behind the run table (`runs` + 65 536).
// PREP >= 64 (BC5_SNORM only): PREP / 16 = TB, the texel bytes of a signed normal source (4, 8 or 16); its ops are the trailing argument
// `sops`, uniform, so each kind is one set of instantiations.  A lane loads two rows of its block (load_rows45 above) and the pair swaps
// codes through a DPP move; everything from P on is the SNORM encoder as it stands.
template <int NCH, bool VEC16, bool WHOLE, bool SGN = false, uint32_t PREP = 0>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(bc45_waves(PREP, WHOLE), bc45_waves(PREP, WHOLE))))
bc45_kernel(const uint8_t* __restrict__ src, int64_t stride, int32_t width, int32_t height, int32_t blocks_x,
            int32_t nlanes, uint8_t* __restrict__ dst, const uint4* __restrict__ runs, uint32_t sops)
{
    constexpr int TB = (int)(PREP >> 4);                          // 0: an RGBA8 surface, a whole block per lane
    constexpr uint32_t BW = TB ? 4u * TB : 16u;                   // bytes of a block's row
    __shared__ StepWeights s_tab[16];                             // [0..7] the 8-step ramp, [8..15] the 6-step ramp
    int32_t lane = blockIdx.x * 256 + threadIdx.x;
    uint32_t w[TB ? 8 * kept_words<TB ? TB : 4>() : 16];
    // WHOLE: block position of this lane and its byte offset from `src`; per chunk both advance by workgroup-uniform steps
    const int32_t step_blocks = (int32_t)gridDim.x * (NCH == 2 ? 128 : 256);
    const int32_t step_y = step_blocks / blocks_x, step_x = step_blocks - step_y * blocks_x;       // scalar, once
    const uint32_t stride32 = (uint32_t)stride;
    int32_t xx = 0;
    uint32_t off = 0;
    auto load_whole = [&](uint32_t o) {
        if constexpr (TB != 0) {                                  // this lane's two rows
#pragma unroll
            for (int r = 0; r < 2; r++)
                load_row45<TB, VEC16>(&w[4 * kept_words<TB>() * r], src + (o + ((threadIdx.x & 1u) * 2u + (uint32_t)r) * stride32));
        } else {
#pragma unroll
            for (int y = 0; y < 4; y++) {
                const uint8_t* p = src + (o + (uint32_t)y * stride32);
                if (VEC16) {
                    const uint4 v = *reinterpret_cast<const uint4*>(p);
                    w[4 * y] = v.x; w[4 * y + 1] = v.y; w[4 * y + 2] = v.z; w[4 * y + 3] = v.w;
                } else {
                    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
                    w[4 * y] = q[0]; w[4 * y + 1] = q[1]; w[4 * y + 2] = q[2]; w[4 * y + 3] = q[3];
                }
            }
        }
    };
    if (WHOLE) {
        const int32_t l0 = lane < nlanes ? lane : nlanes - 1;
        const int32_t b0 = (NCH == 2) ? (l0 >> 1) : l0;
        const int32_t yy = b0 / blocks_x;
        xx = b0 - yy * blocks_x;
        off = (uint32_t)yy * 4u * stride32 + (uint32_t)xx * BW;
        load_whole(off);
    } else if constexpr (TB == 0) {
        load_words45<NCH, VEC16>(w, src, stride, width, height, blocks_x, lane < nlanes ? lane : nlanes - 1);
    }
    if (threadIdx.x < 16) s_tab[threadIdx.x] = step_weights(threadIdx.x < 8 ? 8 : 6, threadIdx.x & 7);
    __syncthreads();
    const uint32_t ch = (NCH == 2) ? (uint32_t)(threadIdx.x & 1) : 0u;   // byte of the RGBA8 word this lane encodes (the grid step is even)
    const uint32_t sel = 0x0c040c00u + ch * 0x00010001u;          // v_perm: byte ch of the first word | byte ch of the second << 16
    const int32_t step = (int32_t)gridDim.x * 256;
    const uint32_t off_step = (uint32_t)step_y * 4u * stride32 + (uint32_t)step_x * BW;
    const uint32_t off_wrap = 4u * stride32 - (uint32_t)blocks_x * BW;            // one block row down, blocks_x blocks back
    for (;;) {
        uint32_t P[8];
        if constexpr (TB != 0) {
            // every lane of the workgroup is here (the loop's exits are uniform), so the neighbour's four dwords arrive by quad_perm [1, 0, 3, 2]
            // (a surface with partial blocks, rare and small, loads here and prefetches nothing: its 64-bit addresses and the texels in flight
            // do not both fit the register budget)
            if (!WHOLE) load_rows45<TB, VEC16>(w, src, stride, width, height, blocks_x, (lane < nlanes ? lane : nlanes - 1) >> 1, (int32_t)ch);
            uint32_t own[4], send[4];
            signed_normal_codes<TB>(own, send, w, ch, sops);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t got = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send[j], 0xb1, 0xf, 0xf, false);
                P[j] = ch ? got : own[j];                         // rows 0, 1: the R lane's own
                P[4 + j] = ch ? own[j] : got;                     // rows 2, 3: the G lane's own
            }
        } else if (PREP & 4u) {
            normalised_codes<PREP>(P, w, ch, reinterpret_cast<const float*>(runs + 65536));
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                P[j] = __builtin_amdgcn_perm(w[2 * j + 1], w[2 * j], sel);
                if (SGN) P[j] = pk_max_u16(P[j] ^ 0x00800080u, 0x00010001u);   // biased; code 0 (int8 -128) becomes code 1 (-127): the same texel, -1.0f
                if (PREP != 0u) P[j] ^= ((PREP >> ch) & 1u) ? 0x00ff00ffu : 0u;  // 255 - code, for the channel this lane encodes
            }
        }
        const int32_t cur = lane;
        lane += step;
        const bool more = (lane - (int32_t)threadIdx.x) < nlanes;         // uniform per workgroup: some lane of the next chunk exists
        if (more) {
            if (WHOLE) {
                xx += step_x; off += off_step;
                if (xx >= blocks_x) { xx -= blocks_x; off += off_wrap; }
                // lanes past the end (last chunk only) re-read the surface's last block: clamp the offset like the lane index
                const uint32_t last = (uint32_t)(height / 4 - 1) * 4u * stride32 + (uint32_t)(blocks_x - 1) * BW;
                load_whole(lane < nlanes ? off : last);
            } else if constexpr (TB == 0) {
                load_words45<NCH, VEC16>(w, src, stride, width, height, blocks_x, lane < nlanes ? lane : nlanes - 1);
            }
        }
        const uint2 o = SGN ? encode_channel_snorm(P, s_tab, s_tab + 8, runs) : encode_channel(P, s_tab, s_tab + 8, runs);
        if (cur < nlanes) *reinterpret_cast<uint2*>(dst + (int64_t)cur * 8) = o;
        if (!more) break;
    }
}

// PREP 1..7 (BC5_UNORM only): the normal-map stages in the load, itwCompressNormalMapBC5; PREP 64 / 128 / 256 (BC5_SNORM only): a signed
// normal source of 4 / 8 / 16-byte texels with the stages `sops`, itwCompressNormalMapBC5S
template <int NCH, bool SGN, uint32_t PREP = 0>
void launch_bc45(const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, hipStream_t st, uint32_t sops = 0)
{
    static_assert(PREP == 0 || (PREP < 8u && NCH == 2 && !SGN) || ((PREP == 64u || PREP == 128u || PREP == 256u) && NCH == 2 && SGN),
                  "the normal-map stages go with BC5_UNORM, a signed normal source with BC5_SNORM");
    if (width <= 0 || height <= 0) return;
    const int bx = (width + 3) / 4, by = (height + 3) / 4;       // DirectXTex keeps partial blocks
    const int64_t n = (int64_t)bx * by * NCH;
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride) & 15) == 0;
    const uint4* runs = index_table<SGN>();
    const int64_t chunks = (n + 255) / 256;
    const dim3 grid((unsigned)(chunks < BC45_GRID ? chunks : BC45_GRID)), blk(256);
    // WHOLE: no partial blocks and every texel offset fits 31 bits, the column term of overlapping rows included (offset32_host.hpp; a
    // positive stride; 16384^2 RGBA8 is 1 GiB).  The stores take 64-bit offsets.
    const bool whole = bc45_walks_32(PREP >= 64u ? (int)(PREP >> 4) : 4, stride, width, height);
    if (whole) {
        if (vec) hipLaunchKernelGGL((bc45_kernel<NCH, true, true, SGN, PREP>),  grid, blk, 0, st, src, stride, width, height, bx, (int32_t)n, dst, runs, sops);
        else     hipLaunchKernelGGL((bc45_kernel<NCH, false, true, SGN, PREP>), grid, blk, 0, st, src, stride, width, height, bx, (int32_t)n, dst, runs, sops);
    } else {
        if (vec) hipLaunchKernelGGL((bc45_kernel<NCH, true, false, SGN, PREP>),  grid, blk, 0, st, src, stride, width, height, bx, (int32_t)n, dst, runs, sops);
        else     hipLaunchKernelGGL((bc45_kernel<NCH, false, false, SGN, PREP>), grid, blk, 0, st, src, stride, width, height, bx, (int32_t)n, dst, runs, sops);
    }
}

// itwCompressNormalMapBC5: PREP is a template argument, so `ops` (1..7) picks one of seven sets of instantiations
template <uint32_t PREP>
void launch_bc5_prep(uint32_t ops, const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, hipStream_t st)
{
    if constexpr (PREP > 7u) fail_msg("BC5 normal map: ops %u", ops);
    else if (ops == PREP) launch_bc45<2, false, PREP>(src, stride, width, height, dst, st);
    else launch_bc5_prep<PREP + 1>(ops, src, stride, width, height, dst, st);
}

#ifdef ITW_TEST_HOOKS
// test hook: closest_indices_snorm for every endpoint pair (one lane each) and every code, sixteen codes per call in biased order, which is
// sixteen consecutive bytes of the pair's 256 once the bias is taken off the position
__global__ void __launch_bounds__(256) bc45_closest_snorm_kernel(uint8_t* __restrict__ out, const uint4* __restrict__ runs)
{
    const uint32_t pair = blockIdx.x * 256u + threadIdx.x, r0 = pair >> 8, r1 = pair & 255u;
    for (uint32_t c = 0; c < 256u; c += 16u) {
        uint32_t P[8], part[2];
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) P[j] = (c + 2u * j) | ((c + 2u * j + 1u) << 16);
        closest_indices_snorm(part, P, r0, r1, runs);
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t bits = part[q >> 1] >> (12 * (q & 1));
            o[q] = (bits & 7u) | (((bits >> 3) & 7u) << 8) | (((bits >> 6) & 7u) << 16) | (((bits >> 9) & 7u) << 24);
        }
        *reinterpret_cast<uint4*>(out + (size_t)pair * 256u + (c ^ 0x80u)) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}
#endif

} // namespace

bool bc45_walks_32(int texel_bytes, int64_t stride, int width, int height)
{
    return (width % 4 == 0) && (height % 4 == 0) && walk_fits_32(stride, width, height, 4 * texel_bytes, 0);
}

void launch_bc4(const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, hipStream_t st) { launch_bc45<1, false>(src, stride, width, height, dst, st); }
void launch_bc5(const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, hipStream_t st) { launch_bc45<2, false>(src, stride, width, height, dst, st); }
void launch_bc4s(const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, hipStream_t st) { launch_bc45<1, true>(src, stride, width, height, dst, st); }
void launch_bc5s(const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, hipStream_t st) { launch_bc45<2, true>(src, stride, width, height, dst, st); }

void launch_bc5_normal(const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, uint32_t ops, hipStream_t st)
{
    if (ops == 0u) launch_bc45<2, false>(src, stride, width, height, dst, st);
    else           launch_bc5_prep<1>(ops, src, stride, width, height, dst, st);
}

void launch_bc5s_normal(const uint8_t* src, int texel_bytes, int64_t stride, int width, int height, uint8_t* dst, uint32_t ops, hipStream_t st)
{
    if (texel_bytes == 4 && ops == 0u) launch_bc45<2, true>(src, stride, width, height, dst, st);      // CompressBlocksBC5S itself
    else if (texel_bytes == 4)  launch_bc45<2, true, 64u>(src, stride, width, height, dst, st, ops);
    else if (texel_bytes == 8)  launch_bc45<2, true, 128u>(src, stride, width, height, dst, st, ops);
    else if (texel_bytes == 16) launch_bc45<2, true, 256u>(src, stride, width, height, dst, st, ops);
    else fail_msg("BC5S normal map: texel_bytes %d", texel_bytes);
}

void warmup_bc45() { (void)index_table<false>(); }
void warmup_bc45s() { (void)index_table<true>(); }

#ifdef ITW_TEST_HOOKS
// test hook (include/itw_test_hooks.h): the run table of the current device, 65 536 entries x 4 words, to host memory
void copy_bc45_index_table(uint32_t* host_out, hipStream_t st)
{
    const uint4* t = index_table<false>();
    ITW_CHECK(hipMemcpyAsync(host_out, t, 65536 * sizeof(uint4), hipMemcpyDeviceToHost, st));
    ITW_CHECK(hipStreamSynchronize(st));
}

// test hook: out[(r0 << 8 | r1) * 256 + code] = the index the SNORM encoders give int8 code `code` (as a byte) under endpoint bytes r0, r1; 16 MiB
void copy_bc45_closest_snorm(uint8_t* host_out, hipStream_t st)
{
    const uint4* t = index_table<true>();
    uint8_t* d = nullptr;
    ITW_CHECK(hipMalloc(&d, (size_t)1 << 24));
    hipLaunchKernelGGL(bc45_closest_snorm_kernel, dim3(256), dim3(256), 0, st, d, t);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host_out, d, (size_t)1 << 24, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(d);
    if (e != hipSuccess) fail_hip("bc45_closest_snorm_kernel", e, __FILE__, __LINE__);
}
#endif

} // namespace itw
