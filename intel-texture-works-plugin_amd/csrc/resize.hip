// resize.hip -- the free-size chain, ITW_MIP_RESIZE (include/itw_dispatch.h, "Mip chains: free sizes"): DirectX::Resize's five non-WIC
// filters (DirectXTexResize.cpp:242-819) between levels whose sizes are the caller's, any ratio per axis, larger or smaller.  The per-axis
// arithmetic is mip_filters.hpp's and mipgen.hpp's, the loads and stores mip_kernels.hpp's; the entry point, its checks and the staging are
// mipgen.hip's (generate_checked, generate_chain).  One launch per level pair, the per-level shape: 64 lanes across, 4 down, grid
// (x tiles, y tiles, items), one lane per texel written.
//   resize_level_kernel   point, box or linear (a template argument).  Point copies the texel at (u * step) >> 16 per axis through the kind's
//                         load and store; box is AVERAGE4 over the 2 x 2 patch, at exactly 2:1 only; linear is _CreateLinearFilter as written,
//                         with its wrap branches, two rows of two taps.
//   resize_cubic_kernel   16 taps straight from memory under clamp, wrap or mirror addressing per axis.  On an upscale neighbouring lanes
//                         share their taps, which L1 serves; the LDS window of mip_cubic_lds_kernel is sized for the chain's 2:1 and is not
//                         used here.
//   triangle              mip_filters.hip's gather (launch_triangle_level) over lists built for the pair: its unrolled path up to six entries
//                         an axis, its general loop above that.  A kernel that staged each source row's span in LDS for the long lists of
//                         4:1 and 16:1 was built and measured against that loop; it took 2.2-2.9 times as long on every row and is not
//                         kept (profiles/resize_timing.jsonl).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
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

enum ResizeMode { RESIZE_POINT = 0, RESIZE_BOX = 1, RESIZE_LINEAR = 2 };

// `wrap`: bit 0 along x, bit 1 along y (read by the linear mode alone); step_x / step_y: mip_point_step (read by the point mode alone)
template <int PX, bool SRGB, int MODE>
__global__ void __launch_bounds__(256)
resize_level_kernel(const MipImage* __restrict__ table, int32_t levels, int32_t dst_level, int32_t sw, int32_t sh, int32_t ow, int32_t oh, float scale_x,
                    float scale_y, uint64_t step_x, uint64_t step_y, uint32_t wrap)
{
    const MipSrgbTables* srgb = mip_srgb_tables<SRGB>();
    const int32_t x = (int32_t)blockIdx.x * 64 + (threadIdx.x & 63), y = (int32_t)blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= ow || y >= oh) return;
    const MipImage* im = table + (int64_t)blockIdx.z * levels + dst_level;
    const MipImage s = im[-1], d = im[0];
    MipTexel t;
    if constexpr (MODE == RESIZE_POINT) {
        const int32_t sx = mip_point_index(x, step_x, sw), sy = mip_point_index(y, step_y, sh);
        t = mip_load<PX, SRGB>(s.ptr + (int64_t)sy * s.stride + (int64_t)sx * PX, srgb);
    } else if constexpr (MODE == RESIZE_BOX) {                            // (sw == 2 * ow and sh == 2 * oh: the launcher's condition)
        const int32_t x0 = min(2 * x, sw - 1), x1 = min(2 * x + 1, sw - 1), y0 = min(2 * y, sh - 1), y1 = min(2 * y + 1, sh - 1);
        const uint8_t* r0 = s.ptr + (int64_t)y0 * s.stride, * r1 = s.ptr + (int64_t)y1 * s.stride;
        t = mip_box(mip_load<PX, SRGB>(r0 + (int64_t)x0 * PX, srgb), mip_load<PX, SRGB>(r1 + (int64_t)x0 * PX, srgb),
                    mip_load<PX, SRGB>(r0 + (int64_t)x1 * PX, srgb), mip_load<PX, SRGB>(r1 + (int64_t)x1 * PX, srgb));
    } else {
        const MipTap tx = mip_linear_tap_wrap(x, scale_x, sw, (wrap & 1u) != 0), ty = mip_linear_tap_wrap(y, scale_y, sh, (wrap & 2u) != 0);
        const uint8_t* r0 = s.ptr + (int64_t)ty.u0 * s.stride, * r1 = s.ptr + (int64_t)ty.u1 * s.stride;
        t = mip_bilinear(mip_load<PX, SRGB>(r0 + (int64_t)tx.u0 * PX, srgb), mip_load<PX, SRGB>(r0 + (int64_t)tx.u1 * PX, srgb),
                         mip_load<PX, SRGB>(r1 + (int64_t)tx.u0 * PX, srgb), mip_load<PX, SRGB>(r1 + (int64_t)tx.u1 * PX, srgb), tx, ty);
    }
    mip_store_row<PX, SRGB, 1>(d.ptr + (int64_t)y * d.stride + (int64_t)x * PX, &t, srgb);
}

// addr_u / addr_v: MipAddress of the axis.  Every tap index comes out of mip_bound_addr, whose last step is the clamp into the row.
template <int PX, bool SRGB>
__global__ void __launch_bounds__(256)
resize_cubic_kernel(const MipImage* __restrict__ table, int32_t levels, int32_t dst_level, int32_t sw, int32_t sh, int32_t ow, int32_t oh, float scale_x,
                    float scale_y, uint32_t addr_u, uint32_t addr_v)
{
    const MipSrgbTables* srgb = mip_srgb_tables<SRGB>();
    const int32_t x = (int32_t)blockIdx.x * 64 + (threadIdx.x & 63), y = (int32_t)blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= ow || y >= oh) return;
    const MipImage* im = table + (int64_t)blockIdx.z * levels + dst_level;
    const MipImage s = im[-1], d = im[0];
    const MipCubicTap tx = mip_cubic_tap_addr(x, scale_x, sw, addr_u), ty = mip_cubic_tap_addr(y, scale_y, sh, addr_v);
    int64_t cx[4];
#pragma unroll
    for (int k = 0; k < 4; k++) cx[k] = (int64_t)mip_bound_addr(tx.b - 1 + k, sw - 1, addr_u) * PX;
    MipTexel c[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint8_t* row = s.ptr + (int64_t)mip_bound_addr(ty.b - 1 + r, sh - 1, addr_v) * s.stride;
        c[r] = mip_cubic(mip_load<PX, SRGB>(row + cx[0], srgb), mip_load<PX, SRGB>(row + cx[1], srgb), mip_load<PX, SRGB>(row + cx[2], srgb),
                         mip_load<PX, SRGB>(row + cx[3], srgb), tx.x);
    }
    MipTexel t = mip_cubic(c[0], c[1], c[2], c[3], ty.x);
    mip_store_row<PX, SRGB, 1, true>(d.ptr + (int64_t)y * d.stride + (int64_t)x * PX, &t, srgb);
}

int resize_pair_filter(const MipFilter& f, int sw, int sh, int ow, int oh)
{
    if (f.kind != MIP_FILTER_DEFAULT) return f.kind;
    return ((int64_t)ow * 2 == sw && (int64_t)oh * 2 == sh) ? MIP_FILTER_BOX : MIP_FILTER_LINEAR;
}

static uint32_t axis_address(bool wrap, bool mirror) { return wrap ? MIP_ADDR_WRAP : mirror ? MIP_ADDR_MIRROR : MIP_ADDR_CLAMP; }   // (wrap wins, as in bounduvw)

template <int PX, bool SRGB>
static void launch_resized(const MipImage* table, const uint32_t* taps, const MipTapPlan& plan, const MipFilter& f, int items, int levels, const int* lw,
                           const int* lh, hipStream_t st)
{
    const uint32_t wrap = (f.wrap_u ? 1u : 0u) | (f.wrap_v ? 2u : 0u);
    for (int l = 1; l < levels; l++) {
        const int sw = lw[l - 1], sh = lh[l - 1], ow = lw[l], oh = lh[l];
        const dim3 grid((unsigned)((ow + 63) / 64), (unsigned)((oh + 3) / 4), (unsigned)items);
        const float scale_x = (float)sw / (float)ow, scale_y = (float)sh / (float)oh;
        const uint64_t step_x = mip_point_step(sw, ow), step_y = mip_point_step(sh, oh);
        switch (resize_pair_filter(f, sw, sh, ow, oh)) {
        case MIP_FILTER_POINT:
            hipLaunchKernelGGL((resize_level_kernel<PX, SRGB, RESIZE_POINT>), grid, dim3(256), 0, st, table, levels, l, sw, sh, ow, oh, scale_x, scale_y, step_x, step_y, wrap);
            break;
        case MIP_FILTER_BOX:
            hipLaunchKernelGGL((resize_level_kernel<PX, SRGB, RESIZE_BOX>), grid, dim3(256), 0, st, table, levels, l, sw, sh, ow, oh, scale_x, scale_y, step_x, step_y, wrap);
            break;
        case MIP_FILTER_LINEAR:
            hipLaunchKernelGGL((resize_level_kernel<PX, SRGB, RESIZE_LINEAR>), grid, dim3(256), 0, st, table, levels, l, sw, sh, ow, oh, scale_x, scale_y, step_x, step_y, wrap);
            break;
        case MIP_FILTER_CUBIC:
            hipLaunchKernelGGL((resize_cubic_kernel<PX, SRGB>), grid, dim3(256), 0, st, table, levels, l, sw, sh, ow, oh, scale_x, scale_y,
                               axis_address(f.wrap_u, f.mirror_u), axis_address(f.wrap_v, f.mirror_v));
            break;
        default:
            launch_triangle_level(table, taps, plan, items, levels, l, ow, oh, PX, SRGB, st);
            break;
        }
        ITW_CHECK(hipGetLastError());
    }
}

void launch_chain_resized(const MipImage* table, const uint32_t* taps, const MipTapPlan& plan, const MipFilter& f, int items, int levels, const int* lw,
                          const int* lh, int px, bool srgb, hipStream_t st)
{
    if (srgb)         launch_resized<4, true>(table, taps, plan, f, items, levels, lw, lh, st);
    else if (px == 4) launch_resized<4, false>(table, taps, plan, f, items, levels, lw, lh, st);
    else              launch_resized<8, false>(table, taps, plan, f, items, levels, lw, lh, st);
}

} // namespace itw

#ifdef ITW_TEST_HOOKS
extern "C" int64_t itwTestResizeTable(int kind, int source, int dest, int address, int32_t* index, float* weight, int64_t capacity)
{
    if (source < 1 || dest < 1 || !index || !weight || address < 0 || address > 2 || capacity < dest) return -1;
    const float scale = (float)source / (float)dest;
    if (kind == itw::MIP_FILTER_POINT) {
        const uint64_t step = itw::mip_point_step(source, dest);
        for (int u = 0; u < dest; u++) { index[u] = itw::mip_point_index(u, step, source); weight[u] = 1.0f; }
        return dest;
    }
    if (kind == itw::MIP_FILTER_LINEAR) {
        if (address == itw::MIP_ADDR_MIRROR) address = itw::MIP_ADDR_CLAMP;       // "mirror is the same case as clamp for linear"
        for (int u = 0; u < dest; u++) {
            const itw::MipTap t = itw::mip_linear_tap_wrap(u, scale, source, address == itw::MIP_ADDR_WRAP);
            index[2 * u] = t.u0; index[2 * u + 1] = t.u1; weight[2 * u] = t.w0; weight[2 * u + 1] = t.w1;
        }
        return dest;
    }
    if (kind == itw::MIP_FILTER_CUBIC) {
        for (int u = 0; u < dest; u++) {
            const itw::MipCubicTap t = itw::mip_cubic_tap_addr(u, scale, source, (uint32_t)address);
            for (int k = 0; k < 4; k++) index[4 * u + k] = itw::mip_bound_addr(t.b - 1 + k, source - 1, (uint32_t)address);
            weight[u] = t.x;
        }
        return dest;
    }
    return -1;
}
#endif
