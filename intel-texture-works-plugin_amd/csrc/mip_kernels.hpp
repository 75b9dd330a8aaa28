// mip_kernels.hpp -- the bodies of the three mip kernels (mipgen.hip's header comment describes them), as force-inlined device templates
// over the texel kind and one more compile-time kind, WEIGHT: alpha-weighted colour (include/itw_dispatch.h, "Mip chains", rule A; RGBA8
// only).  mipgen.hip instantiates them with WEIGHT = false under the names mip_*_kernel<PX, SRGB>, mip_alpha.hip with WEIGHT = true under
// names of its own; the launch sequence of a chain (launch_chain) is here as well, over whichever four kernels it is handed.
// WEIGHT changes one thing: the filter call.  What is kept in registers and LDS between the levels stays the stored texel, widened, so each
// level is premultiplied afresh from what was stored, and loads, stores, routes and LDS layouts are the plain kinds'.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <vector>
#include "mipgen.hpp"
#include "host_rt.hpp"

namespace itw {

// one image of a chain; the table holds items * levels of them in DDS order (item-major, then level)
struct MipImage { uint8_t* ptr; int64_t stride; };

// N consecutive texels at `p` (PX aligned): one vector access where the address allows, texel by texel otherwise
template <int PX, bool SRGB, int N>
__device__ __forceinline__ void mip_load_row(const uint8_t* p, MipTexel* t, const MipSrgbTables* srgb)
{
    constexpr int W = N * PX / 4;
    uint32_t w[W];
    if (W >= 4 && ((uintptr_t)p & 15) == 0) {
#pragma unroll
        for (int i = 0; i < W / 4; i++) {
            const uint4 v = reinterpret_cast<const uint4*>(p)[i];
            w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
        }
    } else if constexpr (PX == 8) {
#pragma unroll
        for (int i = 0; i < N; i++) { const uint2 v = reinterpret_cast<const uint2*>(p)[i]; w[2 * i] = v.x; w[2 * i + 1] = v.y; }
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) w[i] = reinterpret_cast<const uint32_t*>(p)[i];
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
        if constexpr (PX == 4) t[i] = mip_widen<4, SRGB>(w[i], 0u, srgb);
        else                   t[i] = mip_widen<8>(w[2 * i], w[2 * i + 1]);
    }
}

template <int PX, bool SRGB>
__device__ __forceinline__ MipTexel mip_load(const uint8_t* p, const MipSrgbTables* srgb)
{
    MipTexel t;
    mip_load_row<PX, SRGB, 1>(p, &t, srgb);
    return t;
}

// one texel's stored words at `p`
template <int PX>
__device__ __forceinline__ void mip_store_words(uint8_t* p, uint32_t lo, uint32_t hi)
{
    if constexpr (PX == 4) *reinterpret_cast<uint32_t*>(p) = lo;
    else                   *reinterpret_cast<uint2*>(p) = make_uint2(lo, hi);
}

// rounds N (1 or 2) consecutive texels to the format and stores them at `p`; `t` becomes the stored values widened
template <int PX, bool SRGB, int N, bool NEG = false>
__device__ __forceinline__ void mip_store_row(uint8_t* p, MipTexel* t, const MipSrgbTables* srgb)
{
    uint32_t lo[N], hi[N];
#pragma unroll
    for (int i = 0; i < N; i++) mip_round<PX, SRGB, NEG>(t[i], lo[i], hi[i], srgb);
    if constexpr (N == 2) {
        if (PX == 8 && ((uintptr_t)p & 15) == 0) { *reinterpret_cast<uint4*>(p) = make_uint4(lo[0], hi[0], lo[1], hi[1]); return; }
        if (PX == 4 && ((uintptr_t)p & 7) == 0)  { *reinterpret_cast<uint2*>(p) = make_uint2(lo[0], lo[1]); return; }
    }
#pragma unroll
    for (int i = 0; i < N; i++) mip_store_words<PX>(p + i * PX, lo[i], hi[i]);
}

// The workgroup's sRGB tables (mipgen.hpp), 2 KiB of LDS beside what the kernel holds there; nothing, and a null pointer, for the other kinds.
// Every lane of the 256 calls it once, before any lane leaves: it ends with a barrier.
template <bool SRGB>
__device__ __forceinline__ const MipSrgbTables* mip_srgb_tables()
{
    if constexpr (SRGB) {
        __shared__ MipSrgbTables tables;
        mip_srgb_fill(&tables);
        return &tables;
    } else {
        return nullptr;
    }
}

// LDS regions of the pyramid kernel, in widened texels: level +2 (16 x 16), +3 (8 x 8), +4 (4 x 4), +5 (2 x 2)
constexpr int kPyrLds = 256 + 64 + 16 + 4;

template <int PX, bool SRGB, bool WEIGHT>
__device__ __forceinline__ void mip_pyramid_body(const MipImage* table, int32_t levels, int32_t src_level, int32_t nout, int32_t tiles_x,
                                                 int32_t tiles_per_item)
{
    __shared__ MipTexel lds[kPyrLds];
    const MipSrgbTables* srgb = mip_srgb_tables<SRGB>();
    const int32_t item = (int32_t)(blockIdx.x / (uint32_t)tiles_per_item);
    const int32_t tile = (int32_t)(blockIdx.x - (uint32_t)item * (uint32_t)tiles_per_item);
    const int32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const MipImage* im = table + (int64_t)item * levels + src_level;      // im[k]: level src_level + k, k <= nout
    const int32_t lx = threadIdx.x & 15, ly = threadIdx.x >> 4;

    MipTexel p[4][4];
    {
        const MipImage s = im[0];
        const uint8_t* src = s.ptr + (int64_t)(ty * 64 + ly * 4) * s.stride + (int64_t)(tx * 64 + lx * 4) * PX;
#pragma unroll
        for (int r = 0; r < 4; r++) mip_load_row<PX, SRGB, 4>(src + r * s.stride, p[r], srgb);
    }
    MipTexel q[2][2];
    {
        const MipImage d = im[1];
        uint8_t* dst = d.ptr + (int64_t)(ty * 32 + ly * 2) * d.stride + (int64_t)(tx * 32 + lx * 2) * PX;
#pragma unroll
        for (int j = 0; j < 2; j++) {
#pragma unroll
            for (int i = 0; i < 2; i++) q[j][i] = mip_box_kind<WEIGHT>(p[2 * j][2 * i], p[2 * j + 1][2 * i], p[2 * j][2 * i + 1], p[2 * j + 1][2 * i + 1]);
            mip_store_row<PX, SRGB, 2>(dst + j * d.stride, q[j], srgb);
        }
    }
    if (nout < 2) return;                                                 // (nout is the launch's: every lane leaves together)
    {
        MipTexel t = mip_box_kind<WEIGHT>(q[0][0], q[1][0], q[0][1], q[1][1]);
        const MipImage d = im[2];
        mip_store_row<PX, SRGB, 1>(d.ptr + (int64_t)(ty * 16 + ly) * d.stride + (int64_t)(tx * 16 + lx) * PX, &t, srgb);
        lds[ly * 16 + lx] = t;
    }
    int32_t from = 0, to = 256;                                           // region offsets: the level read, the level written
#pragma unroll
    for (int k = 3; k <= 6; k++) {
        if (nout < k) return;
        __syncthreads();
        const int32_t n = 64 >> k;                                        // 8, 4, 2, 1 texels across the tile at level +k
        if ((int32_t)threadIdx.x < n * n) {
            const int32_t x = threadIdx.x & (n - 1), y = threadIdx.x / n;
            const MipTexel* s = lds + from + (2 * y) * (2 * n) + 2 * x;
            MipTexel t = mip_box_kind<WEIGHT>(s[0], s[2 * n], s[1], s[2 * n + 1]);
            const MipImage d = im[k];
            mip_store_row<PX, SRGB, 1>(d.ptr + (int64_t)(ty * n + y) * d.stride + (int64_t)(tx * n + x) * PX, &t, srgb);
            if (k < 6) lds[to + y * n + x] = t;
        }
        from = to; to += n * n;
    }
}

// source level `src_level` of w x h, powers of two, at most 64 x 32 or 32 x 64 (launch_chain gives 64 x 64 to the pyramid kernel); one
// workgroup per item, `nout` levels down.  Levels live in LDS as stored words: odd ones (+1 <= 512 texels, +3, +5) in buf_a, even ones
// (+2 <= 128 texels, +4, +6) in buf_b; the barrier that ends a level also ends the reads of the buffer the next level overwrites.
template <int PX, bool SRGB, bool WEIGHT>
__device__ __forceinline__ void mip_tail_body(const MipImage* table, int32_t levels, int32_t src_level, int32_t nout, int32_t w, int32_t h)
{
    __shared__ uint2 buf_a[512], buf_b[128];
    const MipSrgbTables* srgb = mip_srgb_tables<SRGB>();
    const MipImage* im = table + (int64_t)blockIdx.x * levels + src_level;
    int32_t sw = w, sh = h;
    for (int k = 1; k <= nout; k++) {
        const int32_t ow = sw > 1 ? sw >> 1 : 1, oh = sh > 1 ? sh >> 1 : 1;
        const uint2* sl = (k & 1) ? buf_b : buf_a;                        // level k - 1 (k >= 2)
        uint2* dl = (k & 1) ? buf_a : buf_b;                              // level k
        const MipImage s = im[k - 1], d = im[k];
        for (int32_t idx = threadIdx.x; idx < ow * oh; idx += 256) {
            const int32_t y = idx / ow, x = idx - y * ow;
            const int32_t x0 = 2 * x, x1 = sw > 1 ? x0 + 1 : x0, y0 = 2 * y, y1 = sh > 1 ? y0 + 1 : y0;
            MipTexel p0, p1, p2, p3;
            if (k == 1) {
                const uint8_t* r0 = s.ptr + y0 * s.stride, * r1 = s.ptr + y1 * s.stride;
                p0 = mip_load<PX, SRGB>(r0 + (int64_t)x0 * PX, srgb); p1 = mip_load<PX, SRGB>(r1 + (int64_t)x0 * PX, srgb);
                p2 = mip_load<PX, SRGB>(r0 + (int64_t)x1 * PX, srgb); p3 = mip_load<PX, SRGB>(r1 + (int64_t)x1 * PX, srgb);
            } else {
                const uint2 a = sl[y0 * sw + x0], b = sl[y1 * sw + x0], c = sl[y0 * sw + x1], e = sl[y1 * sw + x1];
                p0 = mip_widen<PX, SRGB>(a.x, a.y, srgb); p1 = mip_widen<PX, SRGB>(b.x, b.y, srgb);
                p2 = mip_widen<PX, SRGB>(c.x, c.y, srgb); p3 = mip_widen<PX, SRGB>(e.x, e.y, srgb);
            }
            MipTexel t = mip_box_kind<WEIGHT>(p0, p1, p2, p3);
            uint32_t lo, hi;
            mip_round<PX, SRGB>(t, lo, hi, srgb);
            mip_store_words<PX>(d.ptr + y * d.stride + (int64_t)x * PX, lo, hi);
            dl[idx] = make_uint2(lo, hi);
        }
        __syncthreads();
        sw = ow; sh = oh;
    }
}

// level `dst_level` (ow x oh) of every item from its level dst_level - 1 (sw x sh); lanes 64 across, 4 down; grid (x tiles, y tiles, items)
template <int PX, bool LINEAR, bool SRGB, bool WEIGHT>
__device__ __forceinline__ void mip_level_body(const MipImage* table, int32_t levels, int32_t dst_level, int32_t sw, int32_t sh, int32_t ow,
                                               int32_t oh, float scale_x, float scale_y)
{
    const MipSrgbTables* srgb = mip_srgb_tables<SRGB>();
    const int32_t x = (int32_t)blockIdx.x * 64 + (threadIdx.x & 63), y = (int32_t)blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= ow || y >= oh) return;
    const MipImage* im = table + (int64_t)blockIdx.z * levels + dst_level;
    const MipImage s = im[-1], d = im[0];
    MipTexel t;
    if (LINEAR) {
        const MipTap tx = mip_linear_tap(x, scale_x, sw), ty = mip_linear_tap(y, scale_y, sh);
        const uint8_t* r0 = s.ptr + (int64_t)ty.u0 * s.stride, * r1 = s.ptr + (int64_t)ty.u1 * s.stride;
        t = mip_bilinear_kind<WEIGHT>(mip_load<PX, SRGB>(r0 + (int64_t)tx.u0 * PX, srgb), mip_load<PX, SRGB>(r0 + (int64_t)tx.u1 * PX, srgb),
                                      mip_load<PX, SRGB>(r1 + (int64_t)tx.u0 * PX, srgb), mip_load<PX, SRGB>(r1 + (int64_t)tx.u1 * PX, srgb), tx, ty);
    } else {
        const int32_t x0 = 2 * x, x1 = sw > 1 ? x0 + 1 : x0, y0 = 2 * y, y1 = sh > 1 ? y0 + 1 : y0;
        const uint8_t* r0 = s.ptr + (int64_t)y0 * s.stride, * r1 = s.ptr + (int64_t)y1 * s.stride;
        t = mip_box_kind<WEIGHT>(mip_load<PX, SRGB>(r0 + (int64_t)x0 * PX, srgb), mip_load<PX, SRGB>(r1 + (int64_t)x0 * PX, srgb),
                                 mip_load<PX, SRGB>(r0 + (int64_t)x1 * PX, srgb), mip_load<PX, SRGB>(r1 + (int64_t)x1 * PX, srgb));
    }
    mip_store_row<PX, SRGB, 1>(d.ptr + (int64_t)y * d.stride + (int64_t)x * PX, &t, srgb);
}

// ---- host: the launches of one chain --------------------------------------------------------------------------------------------------

inline int mip_dim(int v, int level) { return std::max(1, v >> std::min(level, 30)); }
inline bool mip_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// the four kernels of one texel kind
struct MipKernels {
    void (*pyramid)(const MipImage*, int32_t, int32_t, int32_t, int32_t, int32_t);
    void (*tail)(const MipImage*, int32_t, int32_t, int32_t, int32_t, int32_t);
    void (*level_box)(const MipImage*, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, float, float);
    void (*level_linear)(const MipImage*, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, float, float);
};

// the launches of one chain: `table` is on the device, the base is w x h, all `items` alike and within the entry points' launch limits
inline void launch_chain(const MipKernels& k, const MipImage* table, int items, int levels, int w, int h, bool per_level, hipStream_t st)
{
    const bool box = mip_pow2(w) && mip_pow2(h);
    int cur = 0;                                                          // the last level that exists
    while (cur < levels - 1) {
        const int sw = mip_dim(w, cur), sh = mip_dim(h, cur);
        if (box && !per_level && sw >= 64 && sh >= 64) {
            const int nout = std::min(6, levels - 1 - cur), tiles_x = sw / 64, tiles = tiles_x * (sh / 64);
            hipLaunchKernelGGL(k.pyramid, dim3((unsigned)(tiles * items)), dim3(256), 0, st, table, levels, cur, nout, tiles_x, tiles);
            cur += nout;
        } else if (box && !per_level && sw <= 64 && sh <= 64) {       // (not both 64: that was a tile)
            hipLaunchKernelGGL(k.tail, dim3((unsigned)items), dim3(256), 0, st, table, levels, cur, levels - 1 - cur, sw, sh);
            cur = levels - 1;
        } else {
            const int ow = mip_dim(w, cur + 1), oh = mip_dim(h, cur + 1);
            const dim3 grid((unsigned)((ow + 63) / 64), (unsigned)((oh + 3) / 4), (unsigned)items);
            const float scale_x = (float)sw / (float)ow, scale_y = (float)sh / (float)oh;
            hipLaunchKernelGGL(box ? k.level_box : k.level_linear, grid, dim3(256), 0, st, table, levels, cur + 1, sw, sh, ow, oh, scale_x, scale_y);
            cur += 1;
        }
        ITW_CHECK(hipGetLastError());
    }
}

// ---- what mipgen.hip (the entry points, the staging) and mip_alpha.hip (the weighted kinds, the coverage passes) need of each other ------

// the weighted RGBA8 kinds' launches of one chain, as launch_chain makes them
void launch_chain_weighted(const MipImage* table, int items, int levels, int w, int h, bool srgb, bool per_level, hipStream_t st);

// Rule B over a generated RGBA8 chain whose table is on the device: histogram, threshold and rescale, three launches behind one another on
// `st` and no host read between them.  `work` is device memory of coverage_work_bytes(items, levels) bytes, 256-B aligned; its report rows
// (items * levels of itw_mip_coverage, DDS order) start at coverage_report_offset(items, levels).
size_t coverage_work_bytes(int items, int levels);
size_t coverage_report_offset(int items, int levels);
void launch_coverage(const MipImage* table, int items, int levels, int w, int h, int ref, uint8_t* work, hipStream_t st);

// ---- mip_filters.hip: ITW_MIP_CUBIC / ITW_MIP_TRIANGLE, one filter on every level, one launch per level ------------------------------------

// a call's filter as its checks left it: kind is mip_filters.hpp's MipFilterKind (0: the default's box or linear, and wrap changes nothing)
// resize: the chain's level sizes are the caller's (ITW_MIP_RESIZE), kind may then be point or linear too and mirror_u / _v may be set
struct MipFilter { int kind = 0; bool wrap_u = false, wrap_v = false, resize = false, mirror_u = false, mirror_v = false; };

// The triangle filter's gather lists of every level and both axes, built on the host: `words` goes to the device behind the chain's image
// table, in the same upload; x_off[l] / y_off[l] are where level l's lists start in it, repeats[l] whether one source reaches one
// destination twice in either (mip_filters.hpp mip_triangle_gather).  Nothing for the other kinds.
struct MipTapPlan {
    std::vector<uint32_t> words, x_off, y_off, repeats;
    std::vector<int> built_for;                                         // wrap_u, wrap_v, then every level's width and height: what `words` holds
    size_t build(const MipFilter& f, int levels, const int* lw, const int* lh);   // lw[l] x lh[l]: level l's size; returns the bytes of `words`
};

// the launches of one filtered chain, any texel kind: `table` and `taps` (the plan's words; unused by the cubic filter) are on the device
void launch_chain_filtered(const MipImage* table, const uint32_t* taps, const MipTapPlan& plan, const MipFilter& f, int items, int levels, int w, int h, int px,
                           bool srgb, hipStream_t st);

// one level of the triangle filter's gather over any (source, dest) pair: level l (ow x oh) of every item from its level l - 1
void launch_triangle_level(const MipImage* table, const uint32_t* taps, const MipTapPlan& plan, int items, int levels, int l, int ow, int oh, int px, bool srgb,
                           hipStream_t st);

// ---- resize.hip: ITW_MIP_RESIZE, a chain whose level sizes are the caller's ------------------------------------------------------------------

// The filter of the level pair (sw x sh) -> (ow x oh) under `f`: f.kind, or for the default DirectX::Resize's choice, box at exactly 2:1
// on both axes and linear otherwise (_PerformResizeUsingCustomFilters).  Returns a MipFilterKind.
int resize_pair_filter(const MipFilter& f, int sw, int sh, int ow, int oh);

// the launches of one free-size chain, any texel kind, one per level: lw[l] x lh[l] is level l's size, `taps` as launch_chain_filtered's
void launch_chain_resized(const MipImage* table, const uint32_t* taps, const MipTapPlan& plan, const MipFilter& f, int items, int levels, const int* lw,
                          const int* lh, int px, bool srgb, hipStream_t st);

} // namespace itw
