// height_normal.hip -- height maps to normal maps (include/itw_dispatch.h, "height maps": ITW_NORMAL_FROM_HEIGHT in the `ops` word of the
// normal-map calls): DirectXTex's ComputeNormalMap as a stage in front of the normal-map stages.  The arithmetic is height_normal_core.hpp's.
//
// One kernel, height_normal_kernel<SRC, DST>, over every image of a call in ONE launch, out of place.  The reference evaluates a row once
// into a float buffer with one wrapped or mirrored entry at either end and keeps three such rows.  Here a workgroup evaluates the heights
// of a 64 x 16 tile and its one-texel halo once into LDS; a lane then owns four consecutive texels of a row (a "quad", as normal_prep.hip),
// reads the 3 rows x 6 columns around them and runs the reference's inner loop four times.  Every column and row index is mapped into the
// image before it is used (hn::neighbour), so nothing outside width x height is read, and a lane stores only the texels of its quad that
// lie inside the row: as dwordx4 at a 16-byte address, texel by texel otherwise.  A second variant, in which every lane loaded and evaluated
// its own window with no LDS, was built, wrote the same bytes and lost on every source kind; it is not kept.
//
// After the stage the bits 0..2 of `ops` apply to the texel in registers with the meaning its convention gives them (normal_prep.hpp).
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstdint>
#include <vector>
#include "../../include/itw_dispatch.h"
#include "../../include/itw_amd.h"
#include "normal_prep.hpp"
#include "height_normal_core.hpp"
#include "host_rt.hpp"
#include "kernels.hpp"

namespace itw {

// One texel from its 3 x 3 heights (rows y - 1, y, y + 1): the stage, then bits 0..2 of `ops` in the target's convention; `o` takes the
// texel's words
template <int DST>
__device__ __forceinline__ void height_normal_texel(const float (&v0)[3], const float (&v1)[3], const float (&v2)[3], uint32_t ops, float amplitude, uint32_t* o)
{
    const hn::Normal t = hn::texel(v0, v1, v2, ops, amplitude, DST == hn::DST_RGBA8);
    if constexpr (DST == hn::DST_RGBA8) {
        const uint32_t w = hn::unorm_code(t.x) | (hn::unorm_code(t.y) << 8) | (hn::unorm_code(t.z) << 16) | (hn::unorm_code(t.a) << 24);
        o[0] = normal_prep_rgba8(w, ops & NORMAL_OPS_ALL);
    } else if constexpr (DST == hn::DST_SNORM8) {
        float v[4] = {t.x, t.y, t.z, t.a};
        normal_signed_ops(v, ops & NORMAL_OPS_ALL);
        o[0] = ((uint32_t)hn::snorm_code(v[0]) & 255u) | (((uint32_t)hn::snorm_code(v[1]) & 255u) << 8)
             | (((uint32_t)hn::snorm_code(v[2]) & 255u) << 16) | ((uint32_t)hn::snorm_code(v[3]) << 24);
    } else if constexpr (DST == hn::DST_HALF) {
        uint32_t lo = hn::half_bits(t.x) | (hn::half_bits(t.y) << 16), hi = hn::half_bits(t.z) | (hn::half_bits(t.a) << 16);
        normal_prep_rgba16f(lo, hi, ops & NORMAL_OPS_ALL);
        o[0] = lo; o[1] = hi;
    } else {                                                      // the signed convention in RGBA16F: a flip negates, which is exact
        const float x = (ops & NORMAL_FLIP_X) ? -t.x : t.x, y = (ops & NORMAL_FLIP_Y) ? -t.y : t.y;
        o[0] = hn::half_bits(x) | (hn::half_bits(y) << 16);
        o[1] = hn::half_bits(t.z) | (hn::half_bits(t.a) << 16);
    }
}

// A workgroup takes a tile of 64 x 16 texels of one image (the tile found in the call's concatenated tile list by binary search over the
// level table; ONE: a call of one image carries its descriptor as the kernel argument `one`), evaluates the heights of the tile and a
// one-texel halo once into 18 x 66 floats (4752 bytes), and every lane then reads its 3 x 6 window from there.
constexpr int HN_TILE_W = 64, HN_TILE_H = 16, HN_LDS_W = HN_TILE_W + 2, HN_LDS_H = HN_TILE_H + 2;
__host__ __device__ inline int64_t height_tiles(int32_t width, int32_t height)
{
    return (int64_t)((width + HN_TILE_W - 1) / HN_TILE_W) * ((height + HN_TILE_H - 1) / HN_TILE_H);
}

template <int SRC, int DST, bool ONE>
__global__ void __launch_bounds__(256)
height_normal_kernel(const HeightLevel* __restrict__ levels, const HeightLevel one, int32_t nlev, uint32_t ops)
{
    constexpr int TB = hn::SrcBytes<SRC>::value, PX = hn::DstBytes<DST>::value;
    __shared__ float tile[HN_LDS_H][HN_LDS_W];
    HeightLevel lv = one;
    if (!ONE) {
        int lo = 0, hi = nlev - 1;                                // the last image whose first tile is <= this workgroup's: uniform
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (levels[mid].first_unit <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
        }
        lv = levels[lo];
    }
    const uint32_t t = (uint32_t)((int64_t)blockIdx.x - lv.first_unit), tiles_x = (uint32_t)((lv.width + HN_TILE_W - 1) / HN_TILE_W);
    const int32_t tile_y = (int32_t)(t / tiles_x), tile_x = (int32_t)(t - (uint32_t)tile_y * tiles_x);
    const int32_t bx = tile_x * HN_TILE_W, by = tile_y * HN_TILE_H;
    const uint32_t channel = hn::ops_channel(ops);
    const bool mirror_u = (ops & hn::MIRROR_U) != 0, mirror_v = (ops & hn::MIRROR_V) != 0;
    for (int i = threadIdx.x; i < HN_LDS_H * HN_LDS_W; i += 256) {
        const int r = i / HN_LDS_W, c = i - r * HN_LDS_W;
        // beyond the image's last column (row) only the first entry is ever read; it and the rest map to an edge, inside the image
        const int32_t x = hn::neighbour(min(bx - 1 + c, lv.width), lv.width, mirror_u), y = hn::neighbour(min(by - 1 + r, lv.height), lv.height, mirror_v);
        tile[r][c] = hn::height_at<SRC>(lv.src + (int64_t)y * lv.src_stride + (int64_t)x * TB, channel);
    }
    __syncthreads();
    const int32_t ty = (int32_t)(threadIdx.x >> 4), qx = (int32_t)(threadIdx.x & 15);
    const int32_t y = by + ty, x0 = bx + 4 * qx;
    if (y >= lv.height || x0 >= lv.width) return;
    const int32_t n = min(4, lv.width - x0);
    const float amplitude = hn::half_float(hn::ops_amplitude_bits(ops));
    uint32_t o[4 * (PX / 4)];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = 4 * qx + k;
        const float v0[3] = {tile[ty][c], tile[ty][c + 1], tile[ty][c + 2]};
        const float v1[3] = {tile[ty + 1][c], tile[ty + 1][c + 1], tile[ty + 1][c + 2]};
        const float v2[3] = {tile[ty + 2][c], tile[ty + 2][c + 1], tile[ty + 2][c + 2]};
        height_normal_texel<DST>(v0, v1, v2, ops, amplitude, o + k * (PX / 4));
    }
    uint8_t* d = lv.dst + (int64_t)y * lv.dst_stride + (int64_t)x0 * PX;
    if (n == 4 && ((uintptr_t)d & 15) == 0) {
#pragma unroll
        for (int k = 0; k < PX / 4; k++) reinterpret_cast<uint4*>(d)[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
    } else {
        uint32_t* d1 = reinterpret_cast<uint32_t*>(d);
#pragma unroll
        for (int k = 0; k < 4 * (PX / 4); k++) if (k < n * (PX / 4)) d1[k] = o[k];
    }
}

// an image's share of a call's work list, in tiles of 64 x 16 texels; and whether one launch (a workgroup per tile) covers a list
int64_t height_units(int width, int height) { return height_tiles(width, height); }
bool height_units_fit(int64_t units) { return units >= 1 && units <= (int64_t)0x7fffffff; }

template <int SRC, int DST>
static void launch_kind(const HeightLevel* d_levels, const HeightLevel& first, int count, int64_t units, uint32_t ops, hipStream_t st)
{
    if (!height_units_fit(units)) fail_msg("launch_height_normal: %lld tiles are more than one launch covers", (long long)units);
    const dim3 grid((unsigned)units), blk(256);
    if (count == 1) hipLaunchKernelGGL((height_normal_kernel<SRC, DST, true>), grid, blk, 0, st, d_levels, first, 1, ops);
    else            hipLaunchKernelGGL((height_normal_kernel<SRC, DST, false>), grid, blk, 0, st, d_levels, first, (int32_t)count, ops);
    ITW_CHECK(hipGetLastError());
}

void launch_height_normal(int src_kind, int dst_kind, const HeightLevel* d_levels, const HeightLevel& first, int count, int64_t units, uint32_t ops, hipStream_t st)
{
    const int pair = src_kind * 8 + dst_kind;
    switch (pair) {
    case hn::SRC_UNORM8 * 8 + hn::DST_RGBA8:       launch_kind<hn::SRC_UNORM8, hn::DST_RGBA8>(d_levels, first, count, units, ops, st); break;
    case hn::SRC_HALF * 8 + hn::DST_HALF:          launch_kind<hn::SRC_HALF, hn::DST_HALF>(d_levels, first, count, units, ops, st); break;
    case hn::SRC_SNORM8 * 8 + hn::DST_SNORM8:      launch_kind<hn::SRC_SNORM8, hn::DST_SNORM8>(d_levels, first, count, units, ops, st); break;
    case hn::SRC_HALF * 8 + hn::DST_SNORM8:        launch_kind<hn::SRC_HALF, hn::DST_SNORM8>(d_levels, first, count, units, ops, st); break;
    case hn::SRC_FLOAT * 8 + hn::DST_SNORM8:       launch_kind<hn::SRC_FLOAT, hn::DST_SNORM8>(d_levels, first, count, units, ops, st); break;
    case hn::SRC_SNORM8 * 8 + hn::DST_HALF_SIGNED: launch_kind<hn::SRC_SNORM8, hn::DST_HALF_SIGNED>(d_levels, first, count, units, ops, st); break;
    case hn::SRC_HALF * 8 + hn::DST_HALF_SIGNED:   launch_kind<hn::SRC_HALF, hn::DST_HALF_SIGNED>(d_levels, first, count, units, ops, st); break;
    case hn::SRC_FLOAT * 8 + hn::DST_HALF_SIGNED:  launch_kind<hn::SRC_FLOAT, hn::DST_HALF_SIGNED>(d_levels, first, count, units, ops, st); break;
    default: fail_msg("launch_height_normal: no kernel from source kind %d to target kind %d", src_kind, dst_kind);
    }
}

int height_signed_source_kind(int texel_bytes) { return texel_bytes == 4 ? hn::SRC_SNORM8 : texel_bytes == 8 ? hn::SRC_HALF : hn::SRC_FLOAT; }

void check_normal_ops(const char* who, uint32_t ops, const char* no_height)
{
    switch (hn::ops_fault(ops)) {
    case hn::OPS_UNKNOWN_BITS: fail_msg("%s: unknown ops bits 0x%x", who, ops);
    case hn::OPS_CHANNEL:      fail_msg("%s: ops 0x%x: height channel %u (0 and 1 red, 2 green, 3 blue, 4 alpha, 5 luminance)", who, ops, hn::ops_channel(ops));
    case hn::OPS_AMPLITUDE:    fail_msg("%s: ops 0x%x: amplitude bits 0x%04x (a finite half above 0: 0x0001 .. 0x7BFF)", who, ops, hn::ops_amplitude_bits(ops));
    default: break;
    }
    if ((ops & hn::FROM_HEIGHT) && no_height) fail_msg("%s: ops 0x%x: ITW_NORMAL_FROM_HEIGHT is not for this call: %s", who, ops, no_height);
}

bool normal_ops_fault(uint32_t ops) { return hn::ops_fault(ops) != hn::OPS_OK; }

void height_level0(int src_kind, int dst_kind, const uint8_t* src, int64_t src_stride, const rgba_surface& level0, uint32_t ops, hipStream_t st)
{
    const HeightLevel lv{src, level0.ptr, src_stride, (int64_t)level0.stride, level0.width, level0.height, 0};
    launch_height_normal(src_kind, dst_kind, nullptr, lv, 1, height_units(level0.width, level0.height), ops, st);
}

// the bytes of an image: from its first texel to the end of its last row
static bool images_overlap(const rgba_surface& a, int a_texel, const rgba_surface& b, int b_texel)
{
    const uintptr_t a0 = (uintptr_t)a.ptr, a1 = a0 + (uintptr_t)(a.height - 1) * (uintptr_t)a.stride + (uintptr_t)a.width * (uintptr_t)a_texel;
    const uintptr_t b0 = (uintptr_t)b.ptr, b1 = b0 + (uintptr_t)(b.height - 1) * (uintptr_t)b.stride + (uintptr_t)b.width * (uintptr_t)b_texel;
    return a0 < b1 && b0 < a1;
}

void height_check_disjoint(const char* who, const rgba_surface* sources, int texel_bytes, const rgba_surface* targets, int count)
{
    for (int t = 0; t < count; t++)
        for (int s = 0; s < count; s++)
            if (images_overlap(targets[t], 4, sources[s], texel_bytes))
                fail_msg("%s: target %d overlaps the bytes of source %d: with ITW_NORMAL_FROM_HEIGHT a texel is made from its neighbours, so no target may be a source", who, t, s);
}

// itwPrepareNormalMapChain with ITW_NORMAL_FROM_HEIGHT: `count` >= 1 images that passed the checks, all of one pointer kind.  In place for
// the caller; the kernel reads a copy of the sources in the thread's ordered buffer and writes the images
void height_prepare_chain(const rgba_surface* im, int count, int px, uint32_t ops, bool dev)
{
    hipStream_t st = (hipStream_t)itwGetStream();
    static thread_local std::vector<HeightLevel> desc;            // grow-only, like the device buffer it is copied into
    desc.resize((size_t)count);
    // the thread's buffer: [level table] [the sources' copies] [staged targets (host pointers)]
    const StagingPlan from(im, count, px, false, count > 1 ? (size_t)count * sizeof(HeightLevel) : 0), to(im, count, px, dev, from.bytes);
    int64_t units = 0;
    for (int i = 0; i < count; i++) units += height_units(im[i].width, im[i].height);
    if (!height_units_fit(units)) fail_msg("itwPrepareNormalMapChain: %lld work units are more than one launch covers", (long long)units);
    uint8_t* base = static_cast<uint8_t*>(decode_scratch(to.bytes, st));
    units = 0;
    for (int i = 0; i < count; i++) {
        desc[(size_t)i] = HeightLevel{from.ptr(i, base), to.ptr(i, base), from.stride(i), to.stride(i), im[i].width, im[i].height, units};
        units += height_units(im[i].width, im[i].height);
        ITW_CHECK(hipMemcpy2DAsync(from.ptr(i, base), (size_t)from.stride(i), im[i].ptr, (size_t)im[i].stride, from.row_bytes(i), (size_t)im[i].height,
                                   dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    }
    if (count > 1) ITW_CHECK(hipMemcpyAsync(base, desc.data(), (size_t)count * sizeof(HeightLevel), hipMemcpyHostToDevice, st));
    const HeightLevel* d_desc = count > 1 ? reinterpret_cast<const HeightLevel*>(base) : nullptr;
    launch_height_normal(px == 4 ? hn::SRC_UNORM8 : hn::SRC_HALF, px == 4 ? hn::DST_RGBA8 : hn::DST_HALF, d_desc, desc[0], count, units, ops, st);
    if (dev) { decode_scratch_done(st); return; }                 // resident: asynchronous on the thread's stream
    download_staged(to, base, st);                                // width x height only: the caller's row padding is not written
    ITW_CHECK(hipStreamSynchronize(st));
    decode_scratch_done(st);
}

// itwQuantizeNormalMapChain with ITW_NORMAL_FROM_HEIGHT: `count` >= 1 pairs that passed the checks, all of one pointer kind
void height_quantize_chain(const rgba_surface* src, int tb, const rgba_surface* dst, int count, uint32_t ops, bool dev)
{
    hipStream_t st = (hipStream_t)itwGetStream();
    static thread_local std::vector<HeightLevel> desc;
    desc.resize((size_t)count);
    // the thread's buffer: [level table] [staged sources] [staged targets] (host pointers)
    const StagingPlan from(src, count, tb, dev, count > 1 ? (size_t)count * sizeof(HeightLevel) : 0), to(dst, count, 4, dev, from.bytes);
    int64_t units = 0;
    for (int i = 0; i < count; i++) units += height_units(src[i].width, src[i].height);
    if (!height_units_fit(units)) fail_msg("itwQuantizeNormalMapChain: %lld work units are more than one launch covers", (long long)units);
    const bool buffer = !dev || count > 1;                        // a resident call of one image touches no buffer of the thread
    uint8_t* base = buffer ? static_cast<uint8_t*>(decode_scratch(to.bytes, st)) : nullptr;
    units = 0;
    for (int i = 0; i < count; i++) {
        desc[(size_t)i] = HeightLevel{from.ptr(i, base), to.ptr(i, base), from.stride(i), to.stride(i), src[i].width, src[i].height, units};
        units += height_units(src[i].width, src[i].height);
    }
    upload_staged(from, base, st);
    if (count > 1) ITW_CHECK(hipMemcpyAsync(base, desc.data(), (size_t)count * sizeof(HeightLevel), hipMemcpyHostToDevice, st));
    const HeightLevel* d_desc = count > 1 ? reinterpret_cast<const HeightLevel*>(base) : nullptr;
    launch_height_normal(height_signed_source_kind(tb), hn::DST_SNORM8, d_desc, desc[0], count, units, ops, st);
    if (dev) { if (buffer) decode_scratch_done(st); return; }     // resident: asynchronous on the thread's stream
    download_staged(to, base, st);
    ITW_CHECK(hipStreamSynchronize(st));
    decode_scratch_done(st);
}

} // namespace itw
