// mipgen.hip -- the fourth stage of the reference's save path, GenerateMipMaps (IntelPlugin.cpp:2112-2146), on the device: DirectXTex's
// non-WIC box and linear 2D filters (include/itw_dispatch.h, "Mip chains"; the arithmetic is mipgen.hpp's), and the save path in one call
// (itwCompressImageMipped).  Level l is filtered from the STORED level l-1, so a chain is a sequence of dependent steps; the work is a
// stream, HBM bound, and its tail levels are launch latency.  Three kernels, all items (cube faces, array slices) in every launch:
//   mip_pyramid_kernel  box.  One workgroup owns a 64 x 64 tile of a source level and writes that tile's part of the next six levels
//                       (32^2 .. 1^2), each rounded to the texel format before the next is formed.  A lane loads a 4 x 4 patch as four row
//                       reads (dwordx4 where the address allows), forms its 2 x 2 of level +1 and its texel of level +2 in registers; levels
//                       +3 .. +6 go through LDS (5.3 KiB) with a barrier each.  No workgroup waits on another: the launch boundary is the
//                       only dependency between tiles.
//   mip_tail_kernel     box.  One workgroup per item takes a source level of at most 64 x 64 (any power-of-two width and height, 1 and
//                       non-square included) down to 1 x 1; levels ping-pong between two LDS buffers of stored words (5 KiB).  A level of
//                       64 x 64 is one tile of the pyramid kernel, so this kernel starts from 64 x 32 or 32 x 64 at the most.
//   mip_level_kernel    box or linear, any size, one launch per level, one lane per texel written: the only route of the linear filter, the
//                       comparison route of the box filter (ITW_MIP_PER_LEVEL), and the bridge of a power-of-two chain whose levels are
//                       neither tileable (an axis below 64) nor small enough for the tail (the other above 64), e.g. 512 x 2.
// A 4096^2 chain is two launches (4096 -> 64 over 4096 tiles, 64 -> 1 over one) where the per-level route takes twelve.
// Every kernel is a template over the texel kind: RGBA8, RGBA16F, and RGBA8 with sRGB colour (ITW_MIP_SRGB; SRGB = true), whose workgroups
// hold the two tables of mipgen.hpp in 2 KiB of LDS -- 256 lanes load them with two coalesced dwords each -- and otherwise take the same
// routes, launches and LDS layouts; the levels kept in registers and LDS between the steps are the stored codes' widened values, as for the others.
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
#include "normal_prep.hpp"
#include "bcn_format.hpp"
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
template <int PX, bool SRGB, int N>
__device__ __forceinline__ void mip_store_row(uint8_t* p, MipTexel* t, const MipSrgbTables* srgb)
{
    uint32_t lo[N], hi[N];
#pragma unroll
    for (int i = 0; i < N; i++) mip_round<PX, SRGB>(t[i], lo[i], hi[i], srgb);
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

template <int PX, bool SRGB>
__global__ void __launch_bounds__(256)
mip_pyramid_kernel(const MipImage* __restrict__ table, int32_t levels, int32_t src_level, int32_t nout, int32_t tiles_x, int32_t tiles_per_item)
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
            for (int i = 0; i < 2; i++) q[j][i] = mip_box(p[2 * j][2 * i], p[2 * j + 1][2 * i], p[2 * j][2 * i + 1], p[2 * j + 1][2 * i + 1]);
            mip_store_row<PX, SRGB, 2>(dst + j * d.stride, q[j], srgb);
        }
    }
    if (nout < 2) return;                                                 // (nout is the launch's: every lane leaves together)
    {
        MipTexel t = mip_box(q[0][0], q[1][0], q[0][1], q[1][1]);
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
            MipTexel t = mip_box(s[0], s[2 * n], s[1], s[2 * n + 1]);
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
template <int PX, bool SRGB>
__global__ void __launch_bounds__(256)
mip_tail_kernel(const MipImage* __restrict__ table, int32_t levels, int32_t src_level, int32_t nout, int32_t w, int32_t h)
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
            MipTexel t = mip_box(p0, p1, p2, p3);
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
template <int PX, bool LINEAR, bool SRGB>
__global__ void __launch_bounds__(256)
mip_level_kernel(const MipImage* __restrict__ table, int32_t levels, int32_t dst_level, int32_t sw, int32_t sh, int32_t ow, int32_t oh,
                 float scale_x, float scale_y)
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
        t = mip_bilinear(mip_load<PX, SRGB>(r0 + (int64_t)tx.u0 * PX, srgb), mip_load<PX, SRGB>(r0 + (int64_t)tx.u1 * PX, srgb),
                         mip_load<PX, SRGB>(r1 + (int64_t)tx.u0 * PX, srgb), mip_load<PX, SRGB>(r1 + (int64_t)tx.u1 * PX, srgb), tx, ty);
    } else {
        const int32_t x0 = 2 * x, x1 = sw > 1 ? x0 + 1 : x0, y0 = 2 * y, y1 = sh > 1 ? y0 + 1 : y0;
        const uint8_t* r0 = s.ptr + (int64_t)y0 * s.stride, * r1 = s.ptr + (int64_t)y1 * s.stride;
        t = mip_box(mip_load<PX, SRGB>(r0 + (int64_t)x0 * PX, srgb), mip_load<PX, SRGB>(r1 + (int64_t)x0 * PX, srgb),
                    mip_load<PX, SRGB>(r0 + (int64_t)x1 * PX, srgb), mip_load<PX, SRGB>(r1 + (int64_t)x1 * PX, srgb));
    }
    mip_store_row<PX, SRGB, 1>(d.ptr + (int64_t)y * d.stride + (int64_t)x * PX, &t, srgb);
}

} // namespace itw

namespace {

inline int mip_dim(int v, int level) { return std::max(1, v >> std::min(level, 30)); }
inline bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// What one launch covers, checked by the entry points before any device work: the per-level kernel's grid has a block row per 4 texel rows
// of level 1 and a plane per item (65 535 each), the pyramid kernel a block per tile and item.
void check_launch_limits(const char* who, int w, int h, int items)
{
    if (items > 65535) itw::fail_msg("%s: %d items are more than one launch covers (65 535)", who, items);
    if (mip_dim(h, 1) > 4 * 65535) itw::fail_msg("%s: a base of %d rows is more than one launch covers (524 280)", who, h);
    if ((int64_t)(w / 64 + 1) * (h / 64 + 1) * items > (int64_t)0x7fffffff) itw::fail_msg("%s: %d items of %d x %d are more tiles than one launch covers", who, items, w, h);
}

// the launches of one chain: `table` is on the device, the base is w x h, all `items` alike and within check_launch_limits
template <int PX, bool SRGB>
void launch_chain(const itw::MipImage* table, int items, int levels, int w, int h, bool per_level, hipStream_t st)
{
    const bool box = pow2(w) && pow2(h);
    int cur = 0;                                                          // the last level that exists
    while (cur < levels - 1) {
        const int sw = mip_dim(w, cur), sh = mip_dim(h, cur);
        if (box && !per_level && sw >= 64 && sh >= 64) {
            const int nout = std::min(6, levels - 1 - cur), tiles_x = sw / 64, tiles = tiles_x * (sh / 64);
            hipLaunchKernelGGL((itw::mip_pyramid_kernel<PX, SRGB>), dim3((unsigned)(tiles * items)), dim3(256), 0, st, table, levels, cur, nout, tiles_x, tiles);
            cur += nout;
        } else if (box && !per_level && sw <= 64 && sh <= 64) {       // (not both 64: that was a tile)
            hipLaunchKernelGGL((itw::mip_tail_kernel<PX, SRGB>), dim3((unsigned)items), dim3(256), 0, st, table, levels, cur, levels - 1 - cur, sw, sh);
            cur = levels - 1;
        } else {
            const int ow = mip_dim(w, cur + 1), oh = mip_dim(h, cur + 1);
            const dim3 grid((unsigned)((ow + 63) / 64), (unsigned)((oh + 3) / 4), (unsigned)items);
            const float scale_x = (float)sw / (float)ow, scale_y = (float)sh / (float)oh;
            if (box) hipLaunchKernelGGL((itw::mip_level_kernel<PX, false, SRGB>), grid, dim3(256), 0, st, table, levels, cur + 1, sw, sh, ow, oh, scale_x, scale_y);
            else     hipLaunchKernelGGL((itw::mip_level_kernel<PX, true, SRGB>), grid, dim3(256), 0, st, table, levels, cur + 1, sw, sh, ow, oh, scale_x, scale_y);
            cur += 1;
        }
        ITW_CHECK(hipGetLastError());
    }
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// everything that needs the device: a chain that passed the checks, all of one pointer kind, levels >= 2
void generate_chain(const rgba_surface* im, int items, int levels, int px, bool srgb, bool per_level, bool dev)
{
    hipStream_t st = (hipStream_t)itwGetStream();
    const int count = items * levels;
    static thread_local std::vector<itw::MipImage> desc;                  // grow-only, like the device buffer it is copied into
    desc.resize((size_t)count);
    // the thread's buffer: [table] [staged images (host pointers), rows of a 16-byte multiple]
    size_t bytes = up256((size_t)count * sizeof(itw::MipImage));
    std::vector<size_t> stage_off(dev ? 0 : (size_t)count);
    for (int i = 0; i < count; i++) {
        desc[(size_t)i].ptr = im[i].ptr; desc[(size_t)i].stride = im[i].stride;
        if (!dev) {
            desc[(size_t)i].stride = (int64_t)(((size_t)im[i].width * px + 15) & ~(size_t)15);
            stage_off[(size_t)i] = bytes;
            bytes += up256((size_t)desc[(size_t)i].stride * (size_t)im[i].height);
        }
    }
    uint8_t* base = static_cast<uint8_t*>(itw::decode_scratch(bytes, st));
    if (!dev)
        for (int i = 0; i < count; i++) {
            desc[(size_t)i].ptr = base + stage_off[(size_t)i];
            if (i % levels == 0)                                          // only the bases go up
                ITW_CHECK(hipMemcpy2DAsync(desc[(size_t)i].ptr, (size_t)desc[(size_t)i].stride, im[i].ptr, (size_t)im[i].stride, (size_t)im[i].width * px,
                                           (size_t)im[i].height, hipMemcpyHostToDevice, st));
        }
    ITW_CHECK(hipMemcpyAsync(base, desc.data(), (size_t)count * sizeof(itw::MipImage), hipMemcpyHostToDevice, st));
    const itw::MipImage* table = reinterpret_cast<const itw::MipImage*>(base);
    if (srgb)         launch_chain<4, true>(table, items, levels, im[0].width, im[0].height, per_level, st);     // (the entry point refused it with px 8)
    else if (px == 4) launch_chain<4, false>(table, items, levels, im[0].width, im[0].height, per_level, st);
    else              launch_chain<8, false>(table, items, levels, im[0].width, im[0].height, per_level, st);
    if (dev) { itw::decode_scratch_done(st); return; }                    // resident: asynchronous on the thread's stream
    for (int i = 0; i < count; i++)                                       // only the written levels come back, width x height only
        if (i % levels != 0)
            ITW_CHECK(hipMemcpy2DAsync(im[i].ptr, (size_t)im[i].stride, desc[(size_t)i].ptr, (size_t)desc[(size_t)i].stride, (size_t)im[i].width * px,
                                       (size_t)im[i].height, hipMemcpyDeviceToHost, st));
    ITW_CHECK(hipStreamSynchronize(st));
    itw::decode_scratch_done(st);
}

// the device-side chain of itwCompressImageMipped: the thread's own grow-only buffer (the staging buffer above is in use by the stages the
// call runs), ordered across streams as host_rt.hpp's decode_scratch is
struct ChainBuffer {
    void* ptr = nullptr; size_t cap = 0; hipEvent_t done = nullptr; hipStream_t stream = nullptr; bool used = false;
    uint8_t* get(size_t bytes, hipStream_t st)
    {
        if (!done) ITW_CHECK(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        if (used && stream != st) ITW_CHECK(hipStreamWaitEvent(st, done, 0));
        if (bytes > cap) {
            if (ptr) { void* old = ptr; ptr = nullptr; cap = 0; ITW_CHECK(hipFree(old)); }      // (waits for the device)
            const size_t want = bytes + bytes / 4 + 4096;
            ITW_CHECK(hipMalloc(&ptr, want));
            cap = want;
        }
        stream = st; used = true;
        return static_cast<uint8_t*>(ptr);
    }
    void release(hipStream_t st) { ITW_CHECK(hipEventRecord(done, st)); }
};
thread_local ChainBuffer t_chain;

} // namespace

namespace itw {

// Level 0 of itwCompressSignedNormalMapMipped: a signed normal base of TB-byte texels (normal_prep.hpp) widened into RGBA16F, the flips of
// `ops` folded in (a negation: exact, and it commutes with both filters).  int8: half(load rule); half: the bits as they are (a flip is the
// sign bit); float: the mip filter's store rule (mip_half_bits).  One lane per texel row quad: 4 * TB bytes in, 32 bytes out, whole vectors
// where the addresses allow.
template <int TB>
__global__ void __launch_bounds__(256)
mip_widen_signed_kernel(const uint8_t* __restrict__ src, int64_t src_stride, uint8_t* __restrict__ dst, int64_t dst_stride, int32_t width, int32_t height, uint32_t ops)
{
    const int32_t qpr = (width + 3) >> 2;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= (int64_t)qpr * height) return;
    const int32_t y = (int32_t)(j / qpr), qx = (int32_t)(j - (int64_t)y * qpr);
    const int32_t n = min(4, width - 4 * qx);
    const uint8_t* s = src + (int64_t)y * src_stride + (int64_t)qx * 4 * TB;
    uint8_t* d = dst + (int64_t)y * dst_stride + (int64_t)qx * 32;
    constexpr int WPT = TB / 4;
    uint32_t w[4 * WPT], o[8];
    if (n == 4 && ((uintptr_t)s & 15) == 0) {
#pragma unroll
        for (int k = 0; k < WPT; k++) { const uint4 t = reinterpret_cast<const uint4*>(s)[k]; w[4 * k] = t.x; w[4 * k + 1] = t.y; w[4 * k + 2] = t.z; w[4 * k + 3] = t.w; }
    } else {
#pragma unroll
        for (int k = 0; k < 4 * WPT; k++) w[k] = k < n * WPT ? reinterpret_cast<const uint32_t*>(s)[k] : 0u;
    }
    const uint32_t flip = ((ops & NORMAL_FLIP_X) ? 0x00008000u : 0u) | ((ops & NORMAL_FLIP_Y) ? 0x80000000u : 0u);   // the sign bits of x and y in the low word
#pragma unroll
    for (int x = 0; x < 4; x++) {
        if (TB == 8) { o[2 * x] = w[2 * x]; o[2 * x + 1] = w[2 * x + 1]; }
        else {
            float v[4];
            normal_load_signed<TB>(v, w + x * WPT);
            o[2 * x] = mip_half_bits(v[0]) | (mip_half_bits(v[1]) << 16);
            o[2 * x + 1] = mip_half_bits(v[2]) | (mip_half_bits(v[3]) << 16);
        }
        o[2 * x] ^= flip;
    }
    if (n == 4 && ((uintptr_t)d & 15) == 0) {
        reinterpret_cast<uint4*>(d)[0] = make_uint4(o[0], o[1], o[2], o[3]);
        reinterpret_cast<uint4*>(d)[1] = make_uint4(o[4], o[5], o[6], o[7]);
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) if (k < 2 * n) reinterpret_cast<uint32_t*>(d)[k] = o[k];
    }
}

} // namespace itw

extern "C" int itwMipLevels(int width, int height)
{
    if (width < 1 || height < 1) return 0;
    int n = 1;
    for (int m = std::max(width, height); m > 1; m >>= 1) n++;
    return n;
}

extern "C" int64_t itwMipChainLayout(int width, int height, int items, int levels, int pixel_size, uint8_t* storage, rgba_surface* out)
{
    const int full = itwMipLevels(width, height);
    if (full == 0 || items < 0 || levels < 0 || levels > full || (pixel_size != 4 && pixel_size != 8)) return -1;
    if ((int64_t)width * pixel_size > (int64_t)0x7fffffff) return -1;     // rgba_surface's stride is an int32
    if (levels == 0) levels = full;
    int64_t off = 0;
    for (int i = 0; i < items; i++)
        for (int l = 0; l < levels; l++) {
            const int w = mip_dim(width, l), h = mip_dim(height, l);
            if (out) {
                rgba_surface& s = out[(size_t)i * levels + l];
                s.ptr = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(storage) + (uintptr_t)off);
                s.width = w; s.height = h; s.stride = w * pixel_size;
            }
            off += (int64_t)w * h * pixel_size;
        }
    return off;
}

extern "C" int itwGenerateMipChain(const rgba_surface* images, int items, int levels, int pixel_size, uint32_t flags)
{
    bool dev = false;
    itw::clear_failure();
    const bool ok = itw::guarded([&] {
        if (pixel_size != 4 && pixel_size != 8) itw::fail_msg("itwGenerateMipChain: pixel_size %d (4: RGBA8, 8: RGBA16F)", pixel_size);
        if (flags & ~(uint32_t)(ITW_MIP_PER_LEVEL | ITW_MIP_SRGB)) itw::fail_msg("itwGenerateMipChain: unknown flag bits 0x%x", flags);
        if ((flags & ITW_MIP_SRGB) && pixel_size != 4) itw::fail_msg("itwGenerateMipChain: ITW_MIP_SRGB is for RGBA8 texels (pixel_size 4): RGBA16F is linear already");
        if (items < 0) itw::fail_msg("itwGenerateMipChain: %d items", items);
        if (items == 0 || levels <= 1) return;
        if (!images) itw::fail_msg("itwGenerateMipChain: null images pointer");
        if ((int64_t)items * levels > (int64_t)0x7fffffff / 64) itw::fail_msg("itwGenerateMipChain: %d items of %d levels", items, levels);
        const int w = images[0].width, h = images[0].height, full = itwMipLevels(w, h);
        if (full == 0) itw::fail_msg("itwGenerateMipChain: the base is %d x %d", w, h);
        if (levels > full) itw::fail_msg("itwGenerateMipChain: %d levels, a full chain of %d x %d has %d", levels, w, h, full);
        check_launch_limits("itwGenerateMipChain", w, h, items);
        for (int i = 0; i < items * levels; i++) {
            const rgba_surface& s = images[i];
            const int item = i / levels, l = i % levels;
            if (!s.ptr) itw::fail_msg("itwGenerateMipChain: item %d level %d has a null texel pointer", item, l);
            if (l == 0 && (s.width != w || s.height != h))
                itw::fail_msg("itwGenerateMipChain: the base of item %d is %d x %d, that of item 0 %d x %d", item, s.width, s.height, w, h);
            if (s.width != mip_dim(w, l) || s.height != mip_dim(h, l))
                itw::fail_msg("itwGenerateMipChain: item %d level %d is %d x %d, the chain's is %d x %d", item, l, s.width, s.height, mip_dim(w, l), mip_dim(h, l));
            if ((int64_t)s.stride < (int64_t)s.width * pixel_size)
                itw::fail_msg("itwGenerateMipChain: item %d level %d: stride %d < %lld bytes per row", item, l, s.stride, (long long)s.width * pixel_size);
            const uintptr_t row_step = s.height > 1 ? (uintptr_t)(uint32_t)s.stride : 0;
            if (((uintptr_t)s.ptr | row_step) & (uintptr_t)(pixel_size - 1))
                itw::fail_msg("itwGenerateMipChain: item %d level %d: texels are not %d-byte aligned", item, l, pixel_size);
        }
        dev = itw::is_device_pointer(images[0].ptr);
        for (int i = 1; i < items * levels; i++)
            if (itw::is_device_pointer(images[i].ptr) != dev)
                itw::fail_msg("itwGenerateMipChain: image %d is %s memory, image 0 %s: all images must be host or all device pointers", i,
                              dev ? "host" : "device", dev ? "device" : "host");
        generate_chain(images, items, levels, pixel_size, (flags & ITW_MIP_SRGB) != 0, (flags & ITW_MIP_PER_LEVEL) != 0, dev);
    });
    return ok ? 0 : -1;
}

// the sRGB colour kind on the host (include/itw_dispatch.h): the tables of srgb_tables.h, E as the counting definition's binary search
extern "C" float itwSrgbToLinear(uint8_t code)
{
    float v;
    std::memcpy(&v, &itw::SRGB_DECODE_BITS[code], sizeof v);
    return v;
}

extern "C" uint8_t itwLinearToSrgb(float v)
{
    uint32_t lo = 0;
    for (uint32_t step = 128; step >= 1; step >>= 1) {                    // lo + step <= 255
        float t;
        std::memcpy(&t, &itw::SRGB_THR_BITS[lo + step], sizeof t);
        if (v >= t) lo += step;
    }
    return (uint8_t)lo;
}

#ifdef ITW_TEST_HOOKS
namespace itw {
__global__ void __launch_bounds__(256)
mip_srgb_encode_test_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, int64_t n)
{
    const MipSrgbTables* srgb = mip_srgb_tables<true>();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (uint8_t)mip_srgb_encode(in[i], srgb);
}
} // namespace itw

extern "C" void itwTestSrgbEncode(const float* d_in, uint8_t* d_out, int64_t n)
{
    itw::clear_failure();
    itw::guarded([&] {
        if (n <= 0) return;
        if (!d_in || !d_out) itw::fail_msg("itwTestSrgbEncode: null pointer");
        if ((n + 255) / 256 > (int64_t)0x7fffffff) itw::fail_msg("itwTestSrgbEncode: %lld values are more than one launch covers", (long long)n);
        hipLaunchKernelGGL(itw::mip_srgb_encode_test_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)itwGetStream(), d_in, d_out, n);
        ITW_CHECK(hipGetLastError());
    });
}
#endif

extern "C" bool itwCompressImageMippedEx(const rgba_surface* bases, int items, int levels, uint32_t normal_ops, uint32_t mip_flags, uint8_t* target,
                                         int dxgi_format, const void* settings, ItwProgressFunc* progress, void* user)
{
    bool done = false;
    itw::clear_failure();
    const bool ok = itw::guarded([&] {
        if (normal_ops & ~7u) itw::fail_msg("itwCompressImageMipped: unknown ops bits 0x%x", normal_ops);
        if (mip_flags & ~(uint32_t)(ITW_MIP_PER_LEVEL | ITW_MIP_SRGB)) itw::fail_msg("itwCompressImageMipped: unknown mip flag bits 0x%x", mip_flags);
        itw::chain_check_with(bases, items, target, dxgi_format, settings);       // counts, null pointers, sizes, strides, format, settings
        const int px = itw::texel_bytes(itw::format_kind(dxgi_format));
        if (mip_flags & ITW_MIP_SRGB) {                                           // colour in RGBA8 codes, or nothing
            if (px != 4) itw::fail_msg("itwCompressImageMipped: ITW_MIP_SRGB with DXGI format %d, whose texels are RGBA16F: linear already", dxgi_format);
            if (dxgi_format == 81 || dxgi_format == 84) itw::fail_msg("itwCompressImageMipped: ITW_MIP_SRGB with DXGI format %d, whose texels are signed codes, not colour", dxgi_format);
            if (normal_ops) itw::fail_msg("itwCompressImageMipped: ITW_MIP_SRGB with normal ops 0x%x: a normal map is not colour", normal_ops);
        }
        const int w = bases[0].width, h = bases[0].height, full = itwMipLevels(w, h);
        for (int i = 0; i < items; i++) {
            if (bases[i].width != w || bases[i].height != h)
                itw::fail_msg("itwCompressImageMipped: base %d is %d x %d, base 0 %d x %d", i, bases[i].width, bases[i].height, w, h);
            const uintptr_t row_step = h > 1 ? (uintptr_t)(uint32_t)bases[i].stride : 0;
            if (((uintptr_t)bases[i].ptr | row_step) & (uintptr_t)(px - 1)) itw::fail_msg("itwCompressImageMipped: base %d: texels are not %d-byte aligned", i, px);
        }
        if (levels < 0 || levels > full) itw::fail_msg("itwCompressImageMipped: %d levels, a full chain of %d x %d has %d", levels, w, h, full);
        if (levels == 0) levels = full;
        if ((int64_t)items * levels > (int64_t)0x7fffffff / 64) itw::fail_msg("itwCompressImageMipped: %d items of %d levels", items, levels);
        check_launch_limits("itwCompressImageMipped", w, h, items);
        const bool dev = itw::is_device_pointer(bases[0].ptr);
        for (int i = 1; i < items; i++)
            if (itw::is_device_pointer(bases[i].ptr) != dev)
                itw::fail_msg("itwCompressImageMipped: base %d is %s memory, base 0 %s: all bases must be host or all device pointers", i,
                              dev ? "host" : "device", dev ? "device" : "host");
        const int64_t bytes = itwMipChainLayout(w, h, items, levels, px, nullptr, nullptr);
        if (bytes < 0) itw::fail_msg("itwCompressImageMipped: a %d x %d base is wider than a surface can describe", w, h);

        hipStream_t st = (hipStream_t)itwGetStream();
        std::vector<rgba_surface> chain((size_t)items * levels), level0((size_t)items);
        itwMipChainLayout(w, h, items, levels, px, t_chain.get((size_t)bytes, st), chain.data());
        for (int i = 0; i < items; i++) {
            level0[(size_t)i] = chain[(size_t)i * levels];
            ITW_CHECK(hipMemcpy2DAsync(level0[(size_t)i].ptr, (size_t)level0[(size_t)i].stride, bases[i].ptr, (size_t)bases[i].stride, (size_t)w * px, (size_t)h,
                                       dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        }
        auto stage = [](int rc, const char* what) { if (rc != 0) itw::fail_msg("itwCompressImageMipped: %s failed: %s", what, itwLastError()); };
        // the reference's order (IntelPlugin.cpp:2103-2152): flip level 0, generate the mips, normalise every level, compress every image
        if (normal_ops & 3u) stage(itwPrepareNormalMapChain(level0.data(), items, px, normal_ops & 3u), "the flip");
        stage(itwGenerateMipChain(chain.data(), items, levels, px, mip_flags), "the mip chain");
        if (normal_ops & 4u) stage(itwPrepareNormalMapChain(chain.data(), items * levels, px, 4u), "the normalise");
        done = itwCompressImageChainEx(chain.data(), items * levels, target, dxgi_format, settings, progress, user);
        t_chain.release(st);
    });
    return ok && done;
}

extern "C" bool itwCompressImageMipped(const rgba_surface* bases, int items, int levels, uint32_t normal_ops, uint8_t* target, int dxgi_format,
                                       const void* settings, ItwProgressFunc* progress, void* user)
{
    return itwCompressImageMippedEx(bases, items, levels, normal_ops, 0, target, dxgi_format, settings, progress, user);
}

// the signed normal-map save path in one call (include/itw_dispatch.h): a composition of the stages, like itwCompressImageMipped
extern "C" bool itwCompressSignedNormalMapMipped(const rgba_surface* bases, int items, int levels, int texel_bytes, uint32_t ops, uint8_t* target,
                                                 int dxgi_format, ItwProgressFunc* progress, void* user)
{
    bool done = false;
    itw::clear_failure();
    const bool ok = itw::guarded([&] {
        if (dxgi_format != 81 && dxgi_format != 84)
            itw::fail_msg("itwCompressSignedNormalMapMipped: DXGI format %d (BC4_SNORM = 81 or BC5_SNORM = 84)", dxgi_format);
        if (texel_bytes != 4 && texel_bytes != 8 && texel_bytes != 16) itw::fail_msg("itwCompressSignedNormalMapMipped: texel_bytes %d (4, 8 or 16)", texel_bytes);
        if (ops & ~7u) itw::fail_msg("itwCompressSignedNormalMapMipped: unknown ops bits 0x%x", ops);
        itw::chain_check_with(bases, items, target, dxgi_format, nullptr);        // counts, null pointers, sizes, format
        const int w = bases[0].width, h = bases[0].height, full = itwMipLevels(w, h);
        for (int i = 0; i < items; i++) {
            if (bases[i].width != w || bases[i].height != h)
                itw::fail_msg("itwCompressSignedNormalMapMipped: base %d is %d x %d, base 0 %d x %d", i, bases[i].width, bases[i].height, w, h);
            if ((int64_t)bases[i].stride < (int64_t)w * texel_bytes)
                itw::fail_msg("itwCompressSignedNormalMapMipped: base %d: stride %d < %lld bytes per row", i, bases[i].stride, (long long)w * texel_bytes);
            const uintptr_t row_step = h > 1 ? (uintptr_t)(uint32_t)bases[i].stride : 0;
            if (((uintptr_t)bases[i].ptr | row_step) & (uintptr_t)(texel_bytes - 1))
                itw::fail_msg("itwCompressSignedNormalMapMipped: base %d: texels are not %d-byte aligned", i, texel_bytes);
        }
        if (levels < 0 || levels > full) itw::fail_msg("itwCompressSignedNormalMapMipped: %d levels, a full chain of %d x %d has %d", levels, w, h, full);
        if (levels == 0) levels = full;
        if ((int64_t)items * levels > (int64_t)0x7fffffff / 64) itw::fail_msg("itwCompressSignedNormalMapMipped: %d items of %d levels", items, levels);
        check_launch_limits("itwCompressSignedNormalMapMipped", w, h, items);
        const bool dev = itw::is_device_pointer(bases[0].ptr);
        for (int i = 1; i < items; i++)
            if (itw::is_device_pointer(bases[i].ptr) != dev)
                itw::fail_msg("itwCompressSignedNormalMapMipped: base %d is %s memory, base 0 %s: all bases must be host or all device pointers", i,
                              dev ? "host" : "device", dev ? "device" : "host");
        const int64_t bytes = itwMipChainLayout(w, h, items, levels, 8, nullptr, nullptr);
        if (bytes < 0) itw::fail_msg("itwCompressSignedNormalMapMipped: a %d x %d base is wider than a surface can describe", w, h);

        // the thread's chain buffer: [RGBA16F chain] [host bases as they are, rows of a 16-byte multiple]
        hipStream_t st = (hipStream_t)itwGetStream();
        const size_t chain_bytes = ((size_t)bytes + 255) & ~(size_t)255, pitch = ((size_t)w * texel_bytes + 15) & ~(size_t)15;
        const size_t base_bytes = dev ? 0 : (pitch * (size_t)h + 255) & ~(size_t)255;
        uint8_t* buf = t_chain.get(chain_bytes + base_bytes * (size_t)items, st);
        std::vector<rgba_surface> chain((size_t)items * levels);
        itwMipChainLayout(w, h, items, levels, 8, buf, chain.data());
        const int64_t quads = (int64_t)((w + 3) >> 2) * h;                        // (within one launch: check_launch_limits bounds the tiles of 64 x 64)
        if ((quads + 255) / 256 > (int64_t)0x7fffffff) itw::fail_msg("itwCompressSignedNormalMapMipped: a %d x %d base is more than one launch covers", w, h);
        const dim3 grid((unsigned)((quads + 255) / 256)), blk(256);
        for (int i = 0; i < items; i++) {
            const uint8_t* src = bases[i].ptr;
            int64_t stride = bases[i].stride;
            if (!dev) {
                uint8_t* staged = buf + chain_bytes + base_bytes * (size_t)i;
                ITW_CHECK(hipMemcpy2DAsync(staged, pitch, bases[i].ptr, (size_t)bases[i].stride, (size_t)w * texel_bytes, (size_t)h, hipMemcpyHostToDevice, st));
                src = staged; stride = (int64_t)pitch;
            }
            const rgba_surface& l0 = chain[(size_t)i * levels];
            if (texel_bytes == 4)      hipLaunchKernelGGL((itw::mip_widen_signed_kernel<4>), grid, blk, 0, st, src, stride, l0.ptr, (int64_t)l0.stride, w, h, ops & 3u);
            else if (texel_bytes == 8) hipLaunchKernelGGL((itw::mip_widen_signed_kernel<8>), grid, blk, 0, st, src, stride, l0.ptr, (int64_t)l0.stride, w, h, ops & 3u);
            else                       hipLaunchKernelGGL((itw::mip_widen_signed_kernel<16>), grid, blk, 0, st, src, stride, l0.ptr, (int64_t)l0.stride, w, h, ops & 3u);
            ITW_CHECK(hipGetLastError());
        }
        if (itwGenerateMipChain(chain.data(), items, levels, 8, 0) != 0) itw::fail_msg("itwCompressSignedNormalMapMipped: the mip chain failed: %s", itwLastError());
        // the normalise runs in fp32 on every level inside the chain's gather: no pass of its own, no rounding to half before the quantisation
        done = itwCompressSignedNormalMapChain(chain.data(), items * levels, 8, target, dxgi_format, ops & 4u, progress, user);
        t_chain.release(st);
    });
    return ok && done;
}
