// mip_filters.hip -- the mip chain's two further filters, ITW_MIP_CUBIC and ITW_MIP_TRIANGLE (include/itw_dispatch.h, "Mip chains: cubic
// and triangle"; the arithmetic is mip_filters.hpp's), with wrap addressing per axis.  One launch per level, the per-level kernel's shape:
// 64 lanes across, 4 down, grid (x tiles, y tiles, items), one lane per texel written, every texel kind through mip_load / mip_store_row.
//   mip_cubic_kernel      16 taps a texel straight from memory: at the chain's 2:1 ratio every source texel is read about four times, from
//                         L1 / L2 after the first.
//   mip_cubic_lds_kernel  the same arithmetic with the workgroup's source window -- at most 132 x 11 texels for its 64 x 4 outputs, wrapped
//                         and clamped while it is staged -- held in LDS as stored words (13 KiB for RGBA16F), so memory is read once.
//                         launch_cubic picks between the two (g_cubic_lds; DESIGN.md 3.11 has the measured rows).
//   mip_triangle_kernel   a gather over the inverted lists of TriangleFilter::_Create (mip_filters.hpp): per output texel the source rows
//                         and columns that reach it, in the reference's order of arrival, acc = texel * (wy * wx) + acc as a multiply and
//                         an add.  The lists of all levels are one block of words behind the chain's image table, uploaded with it.
// The store is the texel kind's own; the raw-code store takes its signed form (mip_byte_signed), since the cubic filter has negative lobes.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>
#include "../../include/itw_dispatch.h"
#include "../../include/itw_amd.h"
#ifdef ITW_TEST_HOOKS
#include "../../include/itw_test_hooks.h"
#endif
#include "mipgen.hpp"
#include "mip_kernels.hpp"
#include "mip_filters.hpp"
#include "host_rt.hpp"

namespace itw {

template <int PX, bool SRGB>
__global__ void __launch_bounds__(256)
mip_cubic_kernel(const MipImage* __restrict__ table, int32_t levels, int32_t dst_level, int32_t sw, int32_t sh, int32_t ow, int32_t oh, float scale_x,
                 float scale_y, uint32_t wrap)
{
    const MipSrgbTables* srgb = mip_srgb_tables<SRGB>();
    const int32_t x = (int32_t)blockIdx.x * 64 + (threadIdx.x & 63), y = (int32_t)blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= ow || y >= oh) return;
    const MipImage* im = table + (int64_t)blockIdx.z * levels + dst_level;
    const MipImage s = im[-1], d = im[0];
    const bool wu = (wrap & 1u) != 0, wv = (wrap & 2u) != 0;
    const MipCubicTap tx = mip_cubic_tap(x, scale_x, sw, wu), ty = mip_cubic_tap(y, scale_y, sh, wv);
    int64_t cx[4];
#pragma unroll
    for (int k = 0; k < 4; k++) cx[k] = (int64_t)mip_bound(tx.b - 1 + k, sw - 1, wu) * PX;
    MipTexel c[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint8_t* row = s.ptr + (int64_t)mip_bound(ty.b - 1 + r, sh - 1, wv) * s.stride;
        c[r] = mip_cubic(mip_load<PX, SRGB>(row + cx[0], srgb), mip_load<PX, SRGB>(row + cx[1], srgb), mip_load<PX, SRGB>(row + cx[2], srgb),
                         mip_load<PX, SRGB>(row + cx[3], srgb), tx.x);
    }
    MipTexel t = mip_cubic(c[0], c[1], c[2], c[3], ty.x);
    mip_store_row<PX, SRGB, 1, true>(d.ptr + (int64_t)y * d.stride + (int64_t)x * PX, &t, srgb);
}

// The source window of a workgroup's 64 x 4 outputs: positions b(first) - 1 .. b(last) + 2 per axis.  b rises by at most scale per output
// and scale <= 2 + 1 / dest, so the window is at most 63 * (2 + 1/64) + 1 + 4 -> 132 wide and 3 * (2 + 1/4) + 1 + 4 -> 11 high; the
// kernel clamps both to the tile all the same, and every tap's index into it.
constexpr int kCubicW = 136, kCubicH = 12;

template <int PX, bool SRGB>
__global__ void __launch_bounds__(256)
mip_cubic_lds_kernel(const MipImage* __restrict__ table, int32_t levels, int32_t dst_level, int32_t sw, int32_t sh, int32_t ow, int32_t oh, float scale_x,
                     float scale_y, uint32_t wrap)
{
    using Word = std::conditional_t<PX == 8, uint2, uint32_t>;
    __shared__ Word tile[kCubicH * kCubicW];
    const MipSrgbTables* srgb = mip_srgb_tables<SRGB>();
    const MipImage* im = table + (int64_t)blockIdx.z * levels + dst_level;
    const MipImage s = im[-1], d = im[0];
    const bool wu = (wrap & 1u) != 0, wv = (wrap & 2u) != 0;
    const int32_t x_first = (int32_t)blockIdx.x * 64, y_first = (int32_t)blockIdx.y * 4;          // (inside the level: the grid is its tiles)
    const int32_t x_last = min(ow - 1, x_first + 63), y_last = min(oh - 1, y_first + 3);
    const int32_t bx0 = mip_cubic_tap(x_first, scale_x, sw, wu).b, by0 = mip_cubic_tap(y_first, scale_y, sh, wv).b;
    const int32_t win_w = min(max(mip_cubic_tap(x_last, scale_x, sw, wu).b - bx0, 0) + 4, kCubicW);
    const int32_t win_h = min(max(mip_cubic_tap(y_last, scale_y, sh, wv).b - by0, 0) + 4, kCubicH);
    for (int32_t idx = threadIdx.x; idx < win_w * win_h; idx += 256) {
        const int32_t r = idx / win_w, c = idx - r * win_w;
        const uint8_t* p = s.ptr + (int64_t)mip_bound(by0 - 1 + r, sh - 1, wv) * s.stride + (int64_t)mip_bound(bx0 - 1 + c, sw - 1, wu) * PX;
        tile[r * kCubicW + c] = *reinterpret_cast<const Word*>(p);
    }
    __syncthreads();
    const int32_t x = x_first + (threadIdx.x & 63), y = y_first + (threadIdx.x >> 6);
    if (x >= ow || y >= oh) return;
    const MipCubicTap tx = mip_cubic_tap(x, scale_x, sw, wu), ty = mip_cubic_tap(y, scale_y, sh, wv);
    const int32_t lx = min(max(tx.b - bx0, 0), kCubicW - 4), ly = min(max(ty.b - by0, 0), kCubicH - 4);
    MipTexel c[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const Word* row = tile + (ly + r) * kCubicW + lx;
        MipTexel p[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if constexpr (PX == 8) p[k] = mip_widen<8>(row[k].x, row[k].y);
            else                   p[k] = mip_widen<4, SRGB>(row[k], 0u, srgb);
        }
        c[r] = mip_cubic(p[0], p[1], p[2], p[3], tx.x);
    }
    MipTexel t = mip_cubic(c[0], c[1], c[2], c[3], ty.x);
    mip_store_row<PX, SRGB, 1, true>(d.ptr + (int64_t)y * d.stride + (int64_t)x * PX, &t, srgb);
}

// `taps` + x_off / y_off: an axis's gather lists (mip_filters.hpp mip_triangle_gather) for this level
template <int PX, bool SRGB>
__global__ void __launch_bounds__(256)
mip_triangle_kernel(const MipImage* __restrict__ table, int32_t levels, int32_t dst_level, int32_t ow, int32_t oh, const uint32_t* __restrict__ taps,
                    uint32_t x_off, uint32_t y_off, uint32_t repeats)
{
    const MipSrgbTables* srgb = mip_srgb_tables<SRGB>();
    const int32_t x = (int32_t)blockIdx.x * 64 + (threadIdx.x & 63), y = (int32_t)blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= ow || y >= oh) return;
    const MipImage* im = table + (int64_t)blockIdx.z * levels + dst_level;
    const MipImage s = im[-1], d = im[0];
    const uint32_t* xs = taps + x_off, * ys = taps + y_off;
    const uint2* xe = reinterpret_cast<const uint2*>(xs + ow + 1), * ye = reinterpret_cast<const uint2*>(ys + oh + 1);   // (8-byte aligned: the host pads)
    const uint32_t x0 = xs[x], x1 = xs[x + 1], y0 = ys[y], y1 = ys[y + 1];
    MipTexel acc;
    acc.c[0] = acc.c[1] = acc.c[2] = acc.c[3] = 0.0f;
    // What nearly every texel takes: at most kTriTaps entries an axis (4 at 2:1, 5 or 6 at 2 + 1/n : 1) and no source twice, so the order
    // of arrival is rows outside, columns inside.  Both lists go into registers up front and the two loops are unrolled under
    // predicates, which lets the loads of a row's texels go out together; the sums stay one chain, in order.
    constexpr uint32_t kTriTaps = 6;
    if (!repeats && x1 - x0 <= kTriTaps && y1 - y0 <= kTriTaps) {
        uint2 ex[kTriTaps], ey[kTriTaps];
#pragma unroll
        for (uint32_t k = 0; k < kTriTaps; k++) {
            ex[k] = x0 + k < x1 ? xe[x0 + k] : make_uint2(0u, 0u);
            ey[k] = y0 + k < y1 ? ye[y0 + k] : make_uint2(0u, 0u);
        }
#pragma unroll
        for (uint32_t j = 0; j < kTriTaps; j++) {
            if (y0 + j < y1) {
                const uint8_t* row = s.ptr + (int64_t)ey[j].x * s.stride;
                const float wy = __uint_as_float(ey[j].y);
#pragma unroll
                for (uint32_t k = 0; k < kTriTaps; k++) {
                    if (x0 + k < x1) {
                        const MipTexel p = mip_load<PX, SRGB>(row + (int64_t)ex[k].x * PX, srgb);
                        const float w = wy * __uint_as_float(ex[k].y);
#pragma unroll
                        for (int ch = 0; ch < 4; ch++) { const float m = p.c[ch] * w; acc.c[ch] = m + acc.c[ch]; }
                    }
                }
            }
        }
        mip_store_row<PX, SRGB, 1, true>(d.ptr + (int64_t)y * d.stride + (int64_t)x * PX, &acc, srgb);
        return;
    }
    for (uint32_t j = y0; j < y1;) {                                      // the entries of one source row: the reference adds them texel by texel
        const uint32_t sy = ye[j].x;
        uint32_t jn = j + 1;
        while (jn < y1 && ye[jn].x == sy) jn++;
        const uint8_t* row = s.ptr + (int64_t)sy * s.stride;
        for (uint32_t k = x0; k < x1;) {
            const uint32_t sx = xe[k].x;
            uint32_t kn = k + 1;
            while (kn < x1 && xe[kn].x == sx) kn++;
            const MipTexel p = mip_load<PX, SRGB>(row + (int64_t)sx * PX, srgb);
            for (uint32_t jj = j; jj < jn; jj++) {
                const float wy = __uint_as_float(ye[jj].y);
                for (uint32_t kk = k; kk < kn; kk++) {
                    const float w = wy * __uint_as_float(xe[kk].y);
#pragma unroll
                    for (int ch = 0; ch < 4; ch++) { const float m = p.c[ch] * w; acc.c[ch] = m + acc.c[ch]; }
                }
            }
            k = kn;
        }
        j = jn;
    }
    mip_store_row<PX, SRGB, 1, true>(d.ptr + (int64_t)y * d.stride + (int64_t)x * PX, &acc, srgb);
}

// which cubic kernel runs; the hooks build can ask for the other (tools/mip_filter_timing.py times them against each other)
bool g_cubic_lds = false;

size_t MipTapPlan::build(const MipFilter& f, int levels, const int* lw, const int* lh)
{
    if (f.kind != MIP_FILTER_TRIANGLE) return 0;
    // the lists depend on nothing else: a run of equal chains builds them once.  Every level's size is in the key: under ITW_MIP_RESIZE
    // two chains of one base and one length may differ in any level below it
    std::vector<int> key = { f.wrap_u ? 1 : 0, f.wrap_v ? 1 : 0 };
    for (int l = 0; l < levels; l++) { key.push_back(lw[l]); key.push_back(lh[l]); }
    if (!words.empty() && key == built_for) return words.size() * sizeof(uint32_t);
    built_for.clear();                                                    // (no chain has an empty key: a build that fails half way matches nothing)
    words.clear(); x_off.assign((size_t)levels, 0u); y_off.assign((size_t)levels, 0u); repeats.assign((size_t)levels, 0u);
    std::vector<MipTriEntry> lists;
    for (int l = 1; l < levels; l++) {
        for (int axis = 0; axis < 2; axis++) {
            const int source = axis ? lh[l - 1] : lw[l - 1], dest = axis ? lh[l] : lw[l];
            mip_triangle_lists(source, dest, axis ? f.wrap_v : f.wrap_u, lists);
            if ((words.size() + (size_t)dest + 1) & 1u) words.push_back(0u);      // the entries, two words each, start on 8 bytes
            if (words.size() + (size_t)dest + 1 + 2 * lists.size() > (size_t)0x7fffffff) fail_msg("mip chain: the triangle filter's lists of a %d x %d base are more than a launch addresses", lw[0], lh[0]);
            (axis ? y_off : x_off)[(size_t)l] = (uint32_t)words.size();
            bool twice = false;
            const bool inside = mip_triangle_gather(lists, dest, words, &twice);
            if (twice) repeats[(size_t)l] = 1u;
            if (!inside) fail_msg("mip chain: the triangle filter's lists of %d -> %d name a destination outside the level", source, dest);
        }
    }
    built_for = key;
    return words.size() * sizeof(uint32_t);
}

template <int PX, bool SRGB>
static void launch_filtered(const MipImage* table, const uint32_t* taps, const MipTapPlan& plan, const MipFilter& f, int items, int levels, int w, int h, hipStream_t st)
{
    for (int l = 1; l < levels; l++) {
        const int sw = mip_dim(w, l - 1), sh = mip_dim(h, l - 1), ow = mip_dim(w, l), oh = mip_dim(h, l);
        const dim3 grid((unsigned)((ow + 63) / 64), (unsigned)((oh + 3) / 4), (unsigned)items);
        if (f.kind == MIP_FILTER_CUBIC) {
            const float scale_x = (float)sw / (float)ow, scale_y = (float)sh / (float)oh;
            const uint32_t wrap = (f.wrap_u ? 1u : 0u) | (f.wrap_v ? 2u : 0u);
            hipLaunchKernelGGL((g_cubic_lds ? mip_cubic_lds_kernel<PX, SRGB> : mip_cubic_kernel<PX, SRGB>), grid, dim3(256), 0, st, table, levels, l, sw, sh, ow, oh,
                               scale_x, scale_y, wrap);
        } else {
            hipLaunchKernelGGL((mip_triangle_kernel<PX, SRGB>), grid, dim3(256), 0, st, table, levels, l, ow, oh, taps, plan.x_off[(size_t)l], plan.y_off[(size_t)l],
                               plan.repeats[(size_t)l]);
        }
        ITW_CHECK(hipGetLastError());
    }
}

void launch_chain_filtered(const MipImage* table, const uint32_t* taps, const MipTapPlan& plan, const MipFilter& f, int items, int levels, int w, int h, int px,
                           bool srgb, hipStream_t st)
{
    if (srgb)         launch_filtered<4, true>(table, taps, plan, f, items, levels, w, h, st);
    else if (px == 4) launch_filtered<4, false>(table, taps, plan, f, items, levels, w, h, st);
    else              launch_filtered<8, false>(table, taps, plan, f, items, levels, w, h, st);
}

// (below launch_filtered, so that the kernels keep the order in the object they had before the free-size chain)
template <int PX, bool SRGB>
static void launch_triangle(const MipImage* table, const uint32_t* taps, const MipTapPlan& plan, int items, int levels, int l, int ow, int oh, hipStream_t st)
{
    const dim3 grid((unsigned)((ow + 63) / 64), (unsigned)((oh + 3) / 4), (unsigned)items);
    hipLaunchKernelGGL((mip_triangle_kernel<PX, SRGB>), grid, dim3(256), 0, st, table, levels, l, ow, oh, taps, plan.x_off[(size_t)l], plan.y_off[(size_t)l],
                       plan.repeats[(size_t)l]);
}

void launch_triangle_level(const MipImage* table, const uint32_t* taps, const MipTapPlan& plan, int items, int levels, int l, int ow, int oh, int px, bool srgb,
                           hipStream_t st)
{
    if (srgb)         launch_triangle<4, true>(table, taps, plan, items, levels, l, ow, oh, st);
    else if (px == 4) launch_triangle<4, false>(table, taps, plan, items, levels, l, ow, oh, st);
    else              launch_triangle<8, false>(table, taps, plan, items, levels, l, ow, oh, st);
    ITW_CHECK(hipGetLastError());
}

} // namespace itw

#ifdef ITW_TEST_HOOKS
extern "C" void itwTestMipCubicVariant(int lds) { itw::g_cubic_lds = lds != 0; }

extern "C" int64_t itwTestMipFilterTable(int kind, int source, int dest, int wrap, int32_t* index, float* weight, int64_t capacity)
{
    if (source < 1 || dest < 1 || !index || !weight) return -1;
    if (kind == itw::MIP_FILTER_CUBIC) {
        if (capacity < dest) return -1;
        const float scale = (float)source / (float)dest;
        for (int u = 0; u < dest; u++) {
            const itw::MipCubicTap t = itw::mip_cubic_tap(u, scale, source, wrap != 0);
            for (int k = 0; k < 4; k++) index[4 * u + k] = itw::mip_bound(t.b - 1 + k, source - 1, wrap != 0);
            weight[u] = t.x;
        }
        return dest;
    }
    if (kind != itw::MIP_FILTER_TRIANGLE) return -1;
    std::vector<itw::MipTriEntry> lists;
    itw::mip_triangle_lists(source, dest, wrap != 0, lists);
    if ((int64_t)lists.size() > capacity) return -1;
    for (size_t i = 0; i < lists.size(); i++) { index[2 * i] = lists[i].from; index[2 * i + 1] = lists[i].to; weight[i] = lists[i].weight; }
    return (int64_t)lists.size();
}
#endif
