// mip3d_kernels.hpp -- the kernels of the volume mip chain (include/itw_dispatch.h, "Mip chains: volumes"): DirectXTex's five 3D filters
// (DirectXTexMipmaps.cpp:1371-2497) over the per-axis arithmetic of mipgen.hpp and mip_filters.hpp and the loads and stores of
// mip_kernels.hpp, so the three texel kinds are the 2D chain's.  One launch per level for every filter: lanes 64 across and 4 down, grid
// (x tiles, y tiles, destination slices), one lane per texel written, no scratch.  The image table holds every slice of the chain in DDS
// volume order (level-major); a launch gets the index of the first slice of its source level and of its destination level.  Once the
// source depth is 1 every kernel takes the reference's 2D form of the same filter, which is the 2D chain's expression over slice 0.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "mipgen.hpp"
#include "mip_kernels.hpp"
#include "mip_filters.hpp"

namespace itw {

// one level pair of a volume chain: the source level is sw x sh x sd from table[src_first], the destination ow x oh x od from table[dst_first]
struct Mip3dLevel { int32_t src_first, dst_first, sw, sh, sd, ow, oh, od; };

// AVERAGE8 (Filters.h:41-51): a[] of slice 2z, b[] of slice 2z+1, each in AVERAGE4's order (x,y), (x,y+1), (x+1,y), (x+1,y+1)
__device__ __forceinline__ MipTexel mip3d_box8(const MipTexel* a, const MipTexel* b)
{
    MipTexel r;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float v = a[0].c[k] + a[1].c[k];
        v = v + a[2].c[k];
        v = v + a[3].c[k];
        v = v + b[0].c[k];
        v = v + b[1].c[k];
        v = v + b[2].c[k];
        v = v + b[3].c[k];
        r.c[k] = v * 0.125f;
    }
    return r;
}

// the four taps of one slice in AVERAGE4's order; an axis of size 1 gives the second tap = the first
template <int PX, bool SRGB>
__device__ __forceinline__ void mip3d_box_taps(const MipImage s, int32_t x, int32_t y, int32_t sw, int32_t sh, MipTexel* p, const MipSrgbTables* srgb)
{
    const int32_t x0 = 2 * x, x1 = sw > 1 ? x0 + 1 : x0, y0 = 2 * y, y1 = sh > 1 ? y0 + 1 : y0;
    const uint8_t* r0 = s.ptr + (int64_t)y0 * s.stride, * r1 = s.ptr + (int64_t)y1 * s.stride;
    p[0] = mip_load<PX, SRGB>(r0 + (int64_t)x0 * PX, srgb); p[1] = mip_load<PX, SRGB>(r1 + (int64_t)x0 * PX, srgb);
    p[2] = mip_load<PX, SRGB>(r0 + (int64_t)x1 * PX, srgb); p[3] = mip_load<PX, SRGB>(r1 + (int64_t)x1 * PX, srgb);
}

template <int PX, bool SRGB>
__global__ void __launch_bounds__(256)
mip3d_box_kernel(const MipImage* __restrict__ table, Mip3dLevel lv)
{
    const MipSrgbTables* srgb = mip_srgb_tables<SRGB>();
    const int32_t x = (int32_t)blockIdx.x * 64 + (threadIdx.x & 63), y = (int32_t)blockIdx.y * 4 + (threadIdx.x >> 6), z = (int32_t)blockIdx.z;
    if (x >= lv.ow || y >= lv.oh) return;
    const MipImage d = table[lv.dst_first + z];
    MipTexel a[4], t;
    if (lv.sd > 1) {
        MipTexel b[4];
        mip3d_box_taps<PX, SRGB>(table[lv.src_first + 2 * z], x, y, lv.sw, lv.sh, a, srgb);
        mip3d_box_taps<PX, SRGB>(table[lv.src_first + 2 * z + 1], x, y, lv.sw, lv.sh, b, srgb);
        t = mip3d_box8(a, b);
    } else {
        mip3d_box_taps<PX, SRGB>(table[lv.src_first], x, y, lv.sw, lv.sh, a, srgb);
        t = mip_box(a[0], a[1], a[2], a[3]);
    }
    mip_store_row<PX, SRGB, 1>(d.ptr + (int64_t)y * d.stride + (int64_t)x * PX, &t, srgb);
}

// _Generate3DMipsPointFilter: 16.16 steps in 64-bit integers per axis; a depth of 1 stays slice 0
template <int PX, bool SRGB>
__global__ void __launch_bounds__(256)
mip3d_point_kernel(const MipImage* __restrict__ table, Mip3dLevel lv)
{
    const MipSrgbTables* srgb = mip_srgb_tables<SRGB>();
    const int32_t x = (int32_t)blockIdx.x * 64 + (threadIdx.x & 63), y = (int32_t)blockIdx.y * 4 + (threadIdx.x >> 6), z = (int32_t)blockIdx.z;
    if (x >= lv.ow || y >= lv.oh) return;
    const int32_t sx = mip_point_index(x, mip_point_step(lv.sw, lv.ow), lv.sw), sy = mip_point_index(y, mip_point_step(lv.sh, lv.oh), lv.sh);
    const int32_t sz = mip_point_index(z, mip_point_step(lv.sd, lv.od), lv.sd);
    const MipImage s = table[lv.src_first + sz], d = table[lv.dst_first + z];
    MipTexel t = mip_load<PX, SRGB>(s.ptr + (int64_t)sy * s.stride + (int64_t)sx * PX, srgb);
    mip_store_row<PX, SRGB, 1>(d.ptr + (int64_t)y * d.stride + (int64_t)x * PX, &t, srgb);
}

// one slice's BILINEAR_INTERPOLATE
template <int PX, bool SRGB>
__device__ __forceinline__ MipTexel mip3d_bilinear_slice(const MipImage s, const MipTap& tx, const MipTap& ty, const MipSrgbTables* srgb)
{
    const uint8_t* r0 = s.ptr + (int64_t)ty.u0 * s.stride, * r1 = s.ptr + (int64_t)ty.u1 * s.stride;
    return mip_bilinear(mip_load<PX, SRGB>(r0 + (int64_t)tx.u0 * PX, srgb), mip_load<PX, SRGB>(r0 + (int64_t)tx.u1 * PX, srgb),
                        mip_load<PX, SRGB>(r1 + (int64_t)tx.u0 * PX, srgb), mip_load<PX, SRGB>(r1 + (int64_t)tx.u1 * PX, srgb), tx, ty);
}

// TRILINEAR_INTERPOLATE (Filters.h:108-112): z.w0 * bilinear(slice u0) + z.w1 * bilinear(slice u1); BILINEAR_INTERPOLATE once depth is 1
template <int PX, bool SRGB>
__global__ void __launch_bounds__(256)
mip3d_linear_kernel(const MipImage* __restrict__ table, Mip3dLevel lv, float scale_x, float scale_y, float scale_z)
{
    const MipSrgbTables* srgb = mip_srgb_tables<SRGB>();
    const int32_t x = (int32_t)blockIdx.x * 64 + (threadIdx.x & 63), y = (int32_t)blockIdx.y * 4 + (threadIdx.x >> 6), z = (int32_t)blockIdx.z;
    if (x >= lv.ow || y >= lv.oh) return;
    const MipImage d = table[lv.dst_first + z];
    const MipTap tx = mip_linear_tap(x, scale_x, lv.sw), ty = mip_linear_tap(y, scale_y, lv.sh);
    MipTexel t;
    if (lv.sd > 1) {
        const MipTap tz = mip_linear_tap(z, scale_z, lv.sd);
        const MipTexel a = mip3d_bilinear_slice<PX, SRGB>(table[lv.src_first + tz.u0], tx, ty, srgb);
        const MipTexel b = mip3d_bilinear_slice<PX, SRGB>(table[lv.src_first + tz.u1], tx, ty, srgb);
#pragma unroll
        for (int k = 0; k < 4; k++) t.c[k] = tz.w0 * a.c[k] + tz.w1 * b.c[k];
    } else {
        t = mip3d_bilinear_slice<PX, SRGB>(table[lv.src_first], tx, ty, srgb);
    }
    mip_store_row<PX, SRGB, 1>(d.ptr + (int64_t)y * d.stride + (int64_t)x * PX, &t, srgb);
}

// one slice of the cubic filter: CUBIC_INTERPOLATE along x for the four y-tap rows, then along y (the 2D chain's expression)
template <int PX, bool SRGB>
__device__ __forceinline__ MipTexel mip3d_cubic_slice(const MipImage s, const int64_t* cx, const int32_t* ry, float fx, float fy, const MipSrgbTables* srgb)
{
    MipTexel c[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint8_t* row = s.ptr + (int64_t)ry[r] * s.stride;
        c[r] = mip_cubic(mip_load<PX, SRGB>(row + cx[0], srgb), mip_load<PX, SRGB>(row + cx[1], srgb), mip_load<PX, SRGB>(row + cx[2], srgb),
                         mip_load<PX, SRGB>(row + cx[3], srgb), fx);
    }
    return mip_cubic(c[0], c[1], c[2], c[3], fy);
}

// _Generate3DMipsCubicFilter: per z tap the slice's x-then-y value D[j], then CUBIC_INTERPOLATE along z (:2091-2109); wrap: bit 0 u, 1 v, 2 w
template <int PX, bool SRGB>
__global__ void __launch_bounds__(256)
mip3d_cubic_kernel(const MipImage* __restrict__ table, Mip3dLevel lv, float scale_x, float scale_y, float scale_z, uint32_t wrap)
{
    const MipSrgbTables* srgb = mip_srgb_tables<SRGB>();
    const int32_t x = (int32_t)blockIdx.x * 64 + (threadIdx.x & 63), y = (int32_t)blockIdx.y * 4 + (threadIdx.x >> 6), z = (int32_t)blockIdx.z;
    if (x >= lv.ow || y >= lv.oh) return;
    const MipImage d = table[lv.dst_first + z];
    const bool wu = (wrap & 1u) != 0, wv = (wrap & 2u) != 0, ww = (wrap & 4u) != 0;
    const MipCubicTap tx = mip_cubic_tap(x, scale_x, lv.sw, wu), ty = mip_cubic_tap(y, scale_y, lv.sh, wv);
    int64_t cx[4];
    int32_t ry[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        cx[k] = (int64_t)mip_bound(tx.b - 1 + k, lv.sw - 1, wu) * PX;
        ry[k] = mip_bound(ty.b - 1 + k, lv.sh - 1, wv);
    }
    MipTexel t;
    if (lv.sd > 1) {
        const MipCubicTap tz = mip_cubic_tap(z, scale_z, lv.sd, ww);
        MipTexel dz[4];
#pragma unroll                                                            // (a rolled loop indexes dz[] at run time, which the compiler answers with 16 KiB of LDS)
        for (int j = 0; j < 4; j++)
            dz[j] = mip3d_cubic_slice<PX, SRGB>(table[lv.src_first + mip_bound(tz.b - 1 + j, lv.sd - 1, ww)], cx, ry, tx.x, ty.x, srgb);
        t = mip_cubic(dz[0], dz[1], dz[2], dz[3], tz.x);
    } else {
        t = mip3d_cubic_slice<PX, SRGB>(table[lv.src_first], cx, ry, tx.x, ty.x, srgb);
    }
    mip_store_row<PX, SRGB, 1, true>(d.ptr + (int64_t)y * d.stride + (int64_t)x * PX, &t, srgb);
}

// _Generate3DMipsTriangleFilter as a gather over the three inverted lists (mip_filters.hpp mip_triangle_gather) of this level: per
// destination texel the source slices, rows and texels that reach it, ascending; within one source texel its z entries outside, then its y
// entries, its x entries inside -- the reference's order of arrival (:2391-2422).  Each term is texel * ((zw * yw) * xw) + acc, a multiply
// and an add.  A depth of 1 has the z list 1 -> 1, whose one weight is 1.0f: (1.0f * yw) * xw is the 2D chain's yw * xw.
template <int PX, bool SRGB>
__global__ void __launch_bounds__(256)
mip3d_triangle_kernel(const MipImage* __restrict__ table, Mip3dLevel lv, const uint32_t* __restrict__ taps, uint32_t x_off, uint32_t y_off, uint32_t z_off)
{
    const MipSrgbTables* srgb = mip_srgb_tables<SRGB>();
    const int32_t x = (int32_t)blockIdx.x * 64 + (threadIdx.x & 63), y = (int32_t)blockIdx.y * 4 + (threadIdx.x >> 6), z = (int32_t)blockIdx.z;
    if (x >= lv.ow || y >= lv.oh) return;
    const MipImage d = table[lv.dst_first + z];
    const uint32_t* xs = taps + x_off, * ys = taps + y_off, * zs = taps + z_off;
    const uint2* xe = reinterpret_cast<const uint2*>(xs + lv.ow + 1), * ye = reinterpret_cast<const uint2*>(ys + lv.oh + 1),
               * ze = reinterpret_cast<const uint2*>(zs + lv.od + 1);                             // (8-byte aligned: the host pads)
    const uint32_t x0 = xs[x], x1 = xs[x + 1], y0 = ys[y], y1 = ys[y + 1], z0 = zs[z], z1 = zs[z + 1];
    MipTexel acc;
    acc.c[0] = acc.c[1] = acc.c[2] = acc.c[3] = 0.0f;
    for (uint32_t i = z0; i < z1;) {                                      // the entries of one source slice
        const uint32_t sz = ze[i].x;
        uint32_t in = i + 1;
        while (in < z1 && ze[in].x == sz) in++;
        const MipImage s = table[lv.src_first + (int32_t)sz];
        for (uint32_t j = y0; j < y1;) {                                  // of one source row
            const uint32_t sy = ye[j].x;
            uint32_t jn = j + 1;
            while (jn < y1 && ye[jn].x == sy) jn++;
            const uint8_t* row = s.ptr + (int64_t)sy * s.stride;
            for (uint32_t k = x0; k < x1;) {                              // of one source texel
                const uint32_t sx = xe[k].x;
                uint32_t kn = k + 1;
                while (kn < x1 && xe[kn].x == sx) kn++;
                const MipTexel p = mip_load<PX, SRGB>(row + (int64_t)sx * PX, srgb);
                for (uint32_t ii = i; ii < in; ii++) {
                    const float wz = __uint_as_float(ze[ii].y);
                    for (uint32_t jj = j; jj < jn; jj++) {
                        const float wzy = wz * __uint_as_float(ye[jj].y);
                        for (uint32_t kk = k; kk < kn; kk++) {
                            const float w = wzy * __uint_as_float(xe[kk].y);
#pragma unroll
                            for (int ch = 0; ch < 4; ch++) { const float m = p.c[ch] * w; acc.c[ch] = m + acc.c[ch]; }
                        }
                    }
                }
                k = kn;
            }
            j = jn;
        }
        i = in;
    }
    mip_store_row<PX, SRGB, 1, true>(d.ptr + (int64_t)y * d.stride + (int64_t)x * PX, &acc, srgb);
}

} // namespace itw
