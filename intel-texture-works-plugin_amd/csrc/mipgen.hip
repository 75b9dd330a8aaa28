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
// The kernels' bodies and the launch sequence of a chain are mip_kernels.hpp's, shared with mip_alpha.hip: the alpha-weighted kinds and the
// coverage passes of itwGenerateMipChainAlpha, whose entry point, checks and staging are this file's (generate_checked, generate_chain).
// With ITW_MIP_CUBIC or ITW_MIP_TRIANGLE the same entry points hand the chain to mip_filters.hip instead: one filter on every level, one
// launch per level, and for the triangle filter the host-built gather lists uploaded behind the image table (generate_chain).
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
#include "mip3d.hpp"
#include "normal_prep.hpp"
#include "bcn_format.hpp"
#include "host_rt.hpp"
#include "height_normal_core.hpp"
#include "kernels.hpp"

namespace itw {

// The plain kinds.  The tail and level kernels' bodies are mip_kernels.hpp's, shared with the alpha-weighted kinds of mip_alpha.hip.  The
// pyramid kernel keeps its body here and mip_kernels.hpp holds a copy for the weighted kind (the filter call is the one difference): as a
// wrapper around the shared body mip_pyramid_kernel<4, false> compiled to 32 VGPRs where it has 29, and tests/test_srgb_mips_cpu.py pins
// the plain kernels' registers, LDS and scratch to what they were.
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

template <int PX, bool SRGB>
__global__ void __launch_bounds__(256)
mip_tail_kernel(const MipImage* __restrict__ table, int32_t levels, int32_t src_level, int32_t nout, int32_t w, int32_t h)
{
    mip_tail_body<PX, SRGB, false>(table, levels, src_level, nout, w, h);
}

template <int PX, bool LINEAR, bool SRGB>
__global__ void __launch_bounds__(256)
mip_level_kernel(const MipImage* __restrict__ table, int32_t levels, int32_t dst_level, int32_t sw, int32_t sh, int32_t ow, int32_t oh,
                 float scale_x, float scale_y)
{
    mip_level_body<PX, LINEAR, SRGB, false>(table, levels, dst_level, sw, sh, ow, oh, scale_x, scale_y);
}

} // namespace itw

namespace {

using itw::mip_dim;

// What one launch covers, checked by the entry points before any device work: the per-level kernel's grid has a block row per 4 texel rows
// of level 1 and a plane per item (65 535 each), the pyramid kernel a block per tile and item.
void check_launch_limits(const char* who, int w, int h, int items)
{
    if (items > 65535) itw::fail_msg("%s: %d items are more than one launch covers (65 535)", who, items);
    if (mip_dim(h, 1) > 4 * 65535) itw::fail_msg("%s: a base of %d rows is more than one launch covers (524 280)", who, h);
    if ((int64_t)(w / 64 + 1) * (h / 64 + 1) * items > (int64_t)0x7fffffff) itw::fail_msg("%s: %d items of %d x %d are more tiles than one launch covers", who, items, w, h);
}

// the launches of one plain chain (mip_kernels.hpp launch_chain): `table` is on the device, all `items` alike and within check_launch_limits
template <int PX, bool SRGB>
void launch_plain_chain(const itw::MipImage* table, int items, int levels, int w, int h, bool per_level, hipStream_t st)
{
    static const itw::MipKernels k = { itw::mip_pyramid_kernel<PX, SRGB>, itw::mip_tail_kernel<PX, SRGB>, itw::mip_level_kernel<PX, false, SRGB>,
                                       itw::mip_level_kernel<PX, true, SRGB> };
    itw::launch_chain(k, table, items, levels, w, h, per_level, st);
}

// the alpha rules of a call, as its checks left them: both off for every call but itwGenerateMipChainAlpha's
struct AlphaRules { bool weight = false; int coverage_ref = 0; itw_mip_coverage* report = nullptr; };

// everything that needs the device: a chain that passed the checks, all of one pointer kind, levels >= 2
void generate_chain(const rgba_surface* im, int items, int levels, int px, bool srgb, bool per_level, bool dev, const AlphaRules& alpha,
                    const itw::MipFilter& filter)
{
    hipStream_t st = (hipStream_t)itwGetStream();
    const int count = items * levels;
    const int w = im[0].width, h = im[0].height;
    int lw[32], lh[32];                                                   // every level's size, as the checks left item 0's (levels <= 32 in either kind of chain)
    for (int l = 0; l < levels; l++) { lw[l] = im[l].width; lh[l] = im[l].height; }
    // what one upload carries: the image table, then the triangle filter's lists (mip_filters.hip) 256-B aligned behind it
    static thread_local std::vector<uint8_t> head;                        // grow-only, like the device buffer it is copied into
    static thread_local itw::MipTapPlan taps;
    const size_t table_bytes = (size_t)count * sizeof(itw::MipImage), taps_off = itw::up256(table_bytes);
    const size_t taps_bytes = taps.build(filter, levels, lw, lh), head_bytes = taps_bytes ? taps_off + taps_bytes : table_bytes;
    head.resize(head_bytes);
    if (taps_bytes) std::memcpy(head.data() + taps_off, taps.words.data(), taps_bytes);
    itw::MipImage* desc = reinterpret_cast<itw::MipImage*>(head.data());
    // the thread's buffer: [table, lists] [the coverage passes' work] [staged images (host pointers)]
    const size_t work_off = itw::up256(head_bytes);
    const itw::StagingPlan plan(im, count, px, dev, work_off + (alpha.coverage_ref ? itw::coverage_work_bytes(items, levels) : 0));
    uint8_t* base = static_cast<uint8_t*>(itw::decode_scratch(plan.bytes, st));
    for (int i = 0; i < count; i++) desc[i] = itw::MipImage{plan.ptr(i, base), plan.stride(i)};
    for (int i = 0; i < count; i += levels) itw::upload_image(plan, base, i, st);                                     // only the bases go up
    ITW_CHECK(hipMemcpyAsync(base, head.data(), head_bytes, hipMemcpyHostToDevice, st));
    const itw::MipImage* table = reinterpret_cast<const itw::MipImage*>(base);
    if (filter.resize) itw::launch_chain_resized(table, reinterpret_cast<const uint32_t*>(base + taps_off), taps, filter, items, levels, lw, lh, px, srgb, st);
    else if (filter.kind)  itw::launch_chain_filtered(table, reinterpret_cast<const uint32_t*>(base + taps_off), taps, filter, items, levels, w, h, px, srgb, st);
    else if (alpha.weight) itw::launch_chain_weighted(table, items, levels, w, h, srgb, per_level, st);              // (RGBA8: the entry point takes no other)
    else if (srgb)    launch_plain_chain<4, true>(table, items, levels, w, h, per_level, st);                        // (the entry point refused it with px 8)
    else if (px == 4) launch_plain_chain<4, false>(table, items, levels, w, h, per_level, st);
    else              launch_plain_chain<8, false>(table, items, levels, w, h, per_level, st);
    if (alpha.coverage_ref) {                                             // over the chain as generated, before anything comes back
        itw::launch_coverage(desc, items, levels, w, h, alpha.coverage_ref, base + work_off, st);
        if (alpha.report)
            ITW_CHECK(hipMemcpyAsync(alpha.report, base + work_off + itw::coverage_report_offset(items, levels), (size_t)count * sizeof(itw_mip_coverage),
                                     hipMemcpyDeviceToHost, st));
    }
    if (dev) {                                                            // resident: asynchronous on the thread's stream, but for a report
        if (alpha.report) ITW_CHECK(hipStreamSynchronize(st));
        itw::decode_scratch_done(st);
        return;
    }
    for (int i = 0; i < count; i++) if (i % levels) itw::download_image(plan, base, i, st);                           // only the written levels come back
    ITW_CHECK(hipStreamSynchronize(st));
    itw::decode_scratch_done(st);
}

// the checks of a call's itw_mip_alpha, which come before every other: `who` names the entry point
AlphaRules check_alpha(const char* who, const itw_mip_alpha* alpha, itw_mip_coverage* report)
{
    AlphaRules r;
    if (alpha) {
        if (alpha->struct_size != sizeof(itw_mip_alpha)) itw::fail_msg("%s: itw_mip_alpha.struct_size %u (%zu)", who, alpha->struct_size, sizeof(itw_mip_alpha));
        if (alpha->reserved != 0) itw::fail_msg("%s: itw_mip_alpha.reserved is 0x%x, not 0", who, alpha->reserved);
        if (alpha->weight_colour > 1) itw::fail_msg("%s: itw_mip_alpha.weight_colour %u (0 or 1)", who, alpha->weight_colour);
        if (alpha->coverage_ref > 255) itw::fail_msg("%s: itw_mip_alpha.coverage_ref %u (1 .. 255, 0: off)", who, alpha->coverage_ref);
        r.weight = alpha->weight_colour == 1;
        r.coverage_ref = (int)alpha->coverage_ref;
    }
    if (report && !r.coverage_ref) itw::fail_msg("%s: a report without coverage_ref: there is nothing to report", who);
    r.report = report;
    return r;
}

// The flag bits of a call, after the alpha checks: `what` is "flag" or "mip flag" as the entry point's messages have it.  Returns the filter.
constexpr uint32_t kMipFlags = ITW_MIP_PER_LEVEL | ITW_MIP_SRGB | ITW_MIP_CUBIC | ITW_MIP_TRIANGLE | ITW_MIP_WRAP_U | ITW_MIP_WRAP_V;
// the bits of the free-size chain: itwGenerateMipChain alone takes them (`resize_call`), every other call refuses them as unknown
constexpr uint32_t kResizeFlags = ITW_MIP_RESIZE | ITW_MIP_POINT | ITW_MIP_LINEAR | ITW_MIP_MIRROR_U | ITW_MIP_MIRROR_V;
itw::MipFilter check_filter_flags(const char* who, const char* what, uint32_t flags, const AlphaRules& alpha, bool resize_call = false)
{
    if (flags & ~(kMipFlags | (resize_call ? kResizeFlags : 0u))) itw::fail_msg("%s: unknown %s bits 0x%x", who, what, flags);
    itw::MipFilter f;
    if ((flags & ITW_MIP_CUBIC) && (flags & ITW_MIP_TRIANGLE)) itw::fail_msg("%s: ITW_MIP_CUBIC and ITW_MIP_TRIANGLE together: a chain takes one filter", who);
    const uint32_t named = flags & (ITW_MIP_POINT | ITW_MIP_LINEAR | ITW_MIP_CUBIC | ITW_MIP_TRIANGLE);
    if (named & (named - 1))
        itw::fail_msg("%s: two filter bits together (0x%x): a chain takes one of ITW_MIP_POINT, ITW_MIP_LINEAR, ITW_MIP_CUBIC and ITW_MIP_TRIANGLE", who, named);
    if (!(flags & ITW_MIP_RESIZE) && (flags & kResizeFlags))
        itw::fail_msg("%s: ITW_MIP_%s without ITW_MIP_RESIZE: the point and linear filters by name and mirror addressing are the free-size chain's", who,
                      (flags & ITW_MIP_POINT) ? "POINT" : (flags & ITW_MIP_LINEAR) ? "LINEAR" : "MIRROR_U / _V");
    f.resize = (flags & ITW_MIP_RESIZE) != 0;
    f.mirror_u = (flags & ITW_MIP_MIRROR_U) != 0; f.mirror_v = (flags & ITW_MIP_MIRROR_V) != 0;
    f.kind = (flags & ITW_MIP_CUBIC) ? itw::MIP_FILTER_CUBIC : (flags & ITW_MIP_TRIANGLE) ? itw::MIP_FILTER_TRIANGLE
           : (flags & ITW_MIP_POINT) ? itw::MIP_FILTER_POINT : (flags & ITW_MIP_LINEAR) ? itw::MIP_FILTER_LINEAR : itw::MIP_FILTER_DEFAULT;
    if (f.kind && alpha.weight)
        itw::fail_msg("%s: weight_colour with ITW_MIP_%s: a quotient of sums with negative weights is no average, and the weighted triangle kind is not built", who,
                      f.kind == itw::MIP_FILTER_CUBIC ? "CUBIC" : "TRIANGLE");
    f.wrap_u = (flags & ITW_MIP_WRAP_U) != 0; f.wrap_v = (flags & ITW_MIP_WRAP_V) != 0;
    return f;
}

// what the coverage rule's 64-bit arithmetic holds: cov0 * n of a level, n <= N0 / 2
void check_coverage_size(const char* who, int w, int h)
{
    if ((int64_t)w * h > ((int64_t)1 << 31)) itw::fail_msg("%s: coverage over a base of %d x %d: more than 2^31 texels", who, w, h);
}

// The image checks of a free-size chain (ITW_MIP_RESIZE; levels >= 2, items >= 1): every level any size >= 1, one size per level across
// the items, every written level within one launch, and no level pair that would take the linear filter's wrap branches on a growing axis.
void check_resized_chain(const char* who, const rgba_surface* images, int items, int levels, int pixel_size, const itw::MipFilter& filter)
{
    if (levels > 32) itw::fail_msg("%s: %d levels under ITW_MIP_RESIZE (2 .. 32)", who, levels);
    if (items > 65535) itw::fail_msg("%s: %d items are more than one launch covers (65 535)", who, items);
    for (int i = 0; i < items * levels; i++) {
        const rgba_surface& s = images[i];
        const int item = i / levels, l = i % levels;
        const itw::ImageFaultKind fault = itw::image_fault(s, pixel_size, pixel_size);          // null texels come before the sizes, the rest after
        if (fault == itw::IMAGE_NULL_TEXELS) itw::fail_image(who, fault, s, pixel_size, pixel_size, "item %d level %d", item, l);
        if (s.width < 1 || s.height < 1) itw::fail_msg("%s: item %d level %d is %d x %d: a level has at least one texel", who, item, l, s.width, s.height);
        if (s.width != images[l].width || s.height != images[l].height)
            itw::fail_msg("%s: item %d level %d is %d x %d, that of item 0 %d x %d: a level has one size across the items", who, item, l, s.width, s.height,
                          images[l].width, images[l].height);
        if (fault) itw::fail_image(who, fault, s, pixel_size, pixel_size, "item %d level %d", item, l);
    }
    for (int l = 1; l < levels; l++) {
        const int sw = images[l - 1].width, sh = images[l - 1].height, ow = images[l].width, oh = images[l].height;
        if (oh > 4 * 65535) itw::fail_msg("%s: level %d of %d rows is more than one launch covers (262 140)", who, l, oh);
        if (itw::resize_pair_filter(filter, sw, sh, ow, oh) != itw::MIP_FILTER_LINEAR) continue;
        const bool grows_u = filter.wrap_u && ow >= sw && sw > 1, grows_v = filter.wrap_v && oh >= sh && sh > 1;
        if (grows_u || grows_v)
            itw::fail_msg("%s: level %d takes the linear filter with ITW_MIP_WRAP_%s where %d texels become %d: the reference forms that axis's last weights "
                          "from the folded index (4 -> 8 ends in r[3] * -3.25 + r[0] * 4.25); ITW_MIP_CUBIC and ITW_MIP_TRIANGLE wrap at any ratio",
                          who, l, grows_u ? "U" : "V", grows_u ? sw : sh, grows_u ? ow : oh);
    }
}

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

namespace {

// itwGenerateMipChain and itwGenerateMipChainAlpha: one set of checks, `who` names the entry point in every message
int generate_checked(const char* who, const rgba_surface* images, int items, int levels, int pixel_size, uint32_t flags, const itw_mip_alpha* alpha_in,
                     itw_mip_coverage* report, bool resize_call)
{
    bool dev = false;
    itw::clear_failure();
    const bool ok = itw::guarded([&] {
        const AlphaRules alpha = check_alpha(who, alpha_in, report);
        if (pixel_size != 4 && pixel_size != 8) itw::fail_msg("%s: pixel_size %d (4: RGBA8, 8: RGBA16F)", who, pixel_size);
        const itw::MipFilter filter = check_filter_flags(who, "flag", flags, alpha, resize_call);
        if ((flags & ITW_MIP_SRGB) && pixel_size != 4) itw::fail_msg("%s: ITW_MIP_SRGB is for RGBA8 texels (pixel_size 4): RGBA16F is linear already", who);
        if (items < 0) itw::fail_msg("%s: %d items", who, items);
        if (items == 0 || levels <= 1) return;
        if (!images) itw::fail_msg("%s: null images pointer", who);
        if ((int64_t)items * levels > (int64_t)0x7fffffff / 64) itw::fail_msg("%s: %d items of %d levels", who, items, levels);
        if (filter.resize) {                                                  // the level sizes are the caller's: "Mip chains: free sizes"
            check_resized_chain(who, images, items, levels, pixel_size, filter);
            dev = itw::all_one_pointer_kind(who, "image", images, items * levels);
            generate_chain(images, items, levels, pixel_size, (flags & ITW_MIP_SRGB) != 0, false, dev, alpha, filter);
            return;
        }
        const int w = images[0].width, h = images[0].height, full = itwMipLevels(w, h);
        if (full == 0) itw::fail_msg("%s: the base is %d x %d", who, w, h);
        if (levels > full) itw::fail_msg("%s: %d levels, a full chain of %d x %d has %d", who, levels, w, h, full);
        check_launch_limits(who, w, h, items);
        if (alpha.coverage_ref) check_coverage_size(who, w, h);
        for (int i = 0; i < items * levels; i++) {
            const rgba_surface& s = images[i];
            const int item = i / levels, l = i % levels;
            const itw::ImageFaultKind fault = itw::image_fault(s, pixel_size, pixel_size);      // null texels come before the sizes, the rest after
            if (fault == itw::IMAGE_NULL_TEXELS) itw::fail_image(who, fault, s, pixel_size, pixel_size, "item %d level %d", item, l);
            if (l == 0 && (s.width != w || s.height != h))
                itw::fail_msg("%s: the base of item %d is %d x %d, that of item 0 %d x %d", who, item, s.width, s.height, w, h);
            if (s.width != mip_dim(w, l) || s.height != mip_dim(h, l))
                itw::fail_msg("%s: item %d level %d is %d x %d, the chain's is %d x %d", who, item, l, s.width, s.height, mip_dim(w, l), mip_dim(h, l));
            if (fault) itw::fail_image(who, fault, s, pixel_size, pixel_size, "item %d level %d", item, l);
        }
        dev = itw::all_one_pointer_kind(who, "image", images, items * levels);
        generate_chain(images, items, levels, pixel_size, (flags & ITW_MIP_SRGB) != 0, (flags & ITW_MIP_PER_LEVEL) != 0, dev, alpha, filter);
    });
    return ok ? 0 : -1;
}

} // namespace

extern "C" int itwGenerateMipChain(const rgba_surface* images, int items, int levels, int pixel_size, uint32_t flags)
{
    if (flags & ITW_MIP_VOLUME)                                           // a volume: `items` is its depth, `images` its slices level-major (mip3d.hip)
        return itw::generate_mip_chain_3d("itwGenerateMipChain", images, items, levels, pixel_size, flags & ~(uint32_t)ITW_MIP_VOLUME);
    return generate_checked("itwGenerateMipChain", images, items, levels, pixel_size, flags, nullptr, nullptr, true);
}

extern "C" int itwGenerateMipChainAlpha(const rgba_surface* images, int items, int levels, uint32_t flags, const itw_mip_alpha* alpha, itw_mip_coverage* report)
{
    return generate_checked("itwGenerateMipChainAlpha", images, items, levels, 4, flags, alpha, report, false);
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

namespace {

// What the one-call saves ask of their bases once chain_check_with has passed them: equal sizes, rows of `texel_bytes` texels aligned to
// their size, `levels` (0: all) within the full chain and the launches' bounds, one pointer kind, and a chain of `chain_px`-byte texels
// that surfaces can describe.
struct MippedBases { int levels; bool dev; int64_t chain_bytes; };
MippedBases check_mipped_bases(const char* who, const rgba_surface* bases, int items, int levels, int texel_bytes, int chain_px)
{
    const int w = bases[0].width, h = bases[0].height, full = itwMipLevels(w, h);
    for (int i = 0; i < items; i++) {
        if (bases[i].width != w || bases[i].height != h) itw::fail_msg("%s: base %d is %d x %d, base 0 %d x %d", who, i, bases[i].width, bases[i].height, w, h);
        if (const itw::ImageFaultKind k = itw::image_fault(bases[i], texel_bytes, texel_bytes)) itw::fail_image(who, k, bases[i], texel_bytes, texel_bytes, "base %d", i);
    }
    if (levels < 0 || levels > full) itw::fail_msg("%s: %d levels, a full chain of %d x %d has %d", who, levels, w, h, full);
    if (levels == 0) levels = full;
    if ((int64_t)items * levels > (int64_t)0x7fffffff / 64) itw::fail_msg("%s: %d items of %d levels", who, items, levels);
    check_launch_limits(who, w, h, items);
    const bool dev = itw::all_one_pointer_kind(who, "base", bases, items);
    const int64_t bytes = itwMipChainLayout(w, h, items, levels, chain_px, nullptr, nullptr);
    if (bytes < 0) itw::fail_msg("%s: a %d x %d base is wider than a surface can describe", who, w, h);
    return MippedBases{levels, dev, bytes};
}

// itwCompressImageMippedEx, and itwCompressImageMippedAlpha when `alpha_call`: the same stages, the alpha rules handed to the generation
bool compress_mipped(const rgba_surface* bases, int items, int levels, uint32_t normal_ops, uint32_t mip_flags, bool alpha_call, const itw_mip_alpha* alpha_in,
                     uint8_t* target, int dxgi_format, const void* settings, ItwProgressFunc* progress, void* user)
{
    bool done = false;
    itw::clear_failure();
    const bool ok = itw::guarded([&] {
        AlphaRules alpha;
        itw::refuse_signed_bc6h(alpha_call ? "itwCompressImageMippedAlpha" : "itwCompressImageMipped", dxgi_format);
        if (alpha_call) {
            alpha = check_alpha("itwCompressImageMippedAlpha", alpha_in, nullptr);
            if (dxgi_format == 95 || dxgi_format == 96) itw::fail_msg("itwCompressImageMippedAlpha: DXGI format %d, whose texels are RGBA16F: the alpha rules are for RGBA8 colour", dxgi_format);
            if (dxgi_format == 81 || dxgi_format == 84) itw::fail_msg("itwCompressImageMippedAlpha: DXGI format %d, whose texels are signed codes, not colour", dxgi_format);
        }
        const bool from_height = (normal_ops & ITW_NORMAL_FROM_HEIGHT) != 0;
        itw::check_normal_ops("itwCompressImageMipped", normal_ops,
                              !from_height ? nullptr
                              : (dxgi_format == 95 || dxgi_format == 96) ? "the format's texels are RGBA16F colour"
                              : (dxgi_format == 81 || dxgi_format == 84) ? "a signed format takes its heights through itwCompressSignedNormalMapMipped" : nullptr);
        if (normal_ops && itw::format_kind(dxgi_format) == itw::BCN_BC1A)
            itw::fail_msg("itwCompressImageMipped: normal ops 0x%x with format 0x%X (BC1 with 1-bit alpha), which holds colour, not normals", normal_ops, dxgi_format);
        if (normal_ops && itw::format_kind(dxgi_format) == itw::BCN_BC3DX)
            itw::fail_msg("itwCompressImageMipped: normal ops 0x%x with format 0x%X (BC3 by DirectXTex's encoder), which holds colour, not normals", normal_ops, dxgi_format);
        if (normal_ops && itw::format_kind(dxgi_format) == itw::BCN_BC2)
            itw::fail_msg("itwCompressImageMipped: normal ops 0x%x with format 0x%X (BC2), which holds colour, not normals", normal_ops, dxgi_format);
        check_filter_flags("itwCompressImageMipped", "mip flag", mip_flags, alpha);
        itw::chain_check_with(bases, items, target, dxgi_format, settings);       // counts, null pointers, sizes, strides, format, settings
        const int px = itw::texel_bytes(itw::format_kind(dxgi_format));
        if (mip_flags & ITW_MIP_SRGB) {                                           // colour in RGBA8 codes, or nothing
            if (px != 4) itw::fail_msg("itwCompressImageMipped: ITW_MIP_SRGB with DXGI format %d, whose texels are RGBA16F: linear already", dxgi_format);
            if (dxgi_format == 81 || dxgi_format == 84) itw::fail_msg("itwCompressImageMipped: ITW_MIP_SRGB with DXGI format %d, whose texels are signed codes, not colour", dxgi_format);
            if (normal_ops) itw::fail_msg("itwCompressImageMipped: ITW_MIP_SRGB with normal ops 0x%x: a normal map is not colour", normal_ops);
        }
        const MippedBases b = check_mipped_bases("itwCompressImageMipped", bases, items, levels, px, px);
        const int w = bases[0].width, h = bases[0].height;
        const bool dev = b.dev;
        levels = b.levels;
        if (alpha.coverage_ref) check_coverage_size("itwCompressImageMippedAlpha", w, h);

        hipStream_t st = (hipStream_t)itwGetStream();
        std::vector<rgba_surface> chain((size_t)items * levels), level0((size_t)items);
        // with ITW_NORMAL_FROM_HEIGHT the thread's chain buffer is [chain] [host bases as they are]: the height stage writes level 0 from the bases
        const itw::StagingPlan heights(bases, items, px, dev || !from_height, (size_t)b.chain_bytes);
        uint8_t* buf = static_cast<uint8_t*>(itw::chain_scratch(from_height ? heights.bytes : (size_t)b.chain_bytes, st));
        itwMipChainLayout(w, h, items, levels, px, buf, chain.data());
        for (int i = 0; i < items; i++) {
            level0[(size_t)i] = chain[(size_t)i * levels];
            if (from_height) {
                itw::upload_image(heights, buf, i, st);
                itw::height_level0(itw::hn::SRC_UNORM8, itw::hn::DST_RGBA8, heights.ptr(i, buf), heights.stride(i), level0[(size_t)i], normal_ops & ~7u, st);
                continue;
            }
            ITW_CHECK(hipMemcpy2DAsync(level0[(size_t)i].ptr, (size_t)level0[(size_t)i].stride, bases[i].ptr, (size_t)bases[i].stride, (size_t)w * px, (size_t)h,
                                       dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        }
        auto stage = [](int rc, const char* what) { if (rc != 0) itw::fail_msg("itwCompressImageMipped: %s failed: %s", what, itwLastError()); };
        // the reference's order (IntelPlugin.cpp:2103-2152): flip level 0, generate the mips, normalise every level, compress every image
        if (normal_ops & 3u) stage(itwPrepareNormalMapChain(level0.data(), items, px, normal_ops & 3u), "the flip");
        if (alpha.weight || alpha.coverage_ref) stage(itwGenerateMipChainAlpha(chain.data(), items, levels, mip_flags, alpha_in, nullptr), "the mip chain");
        else                                    stage(itwGenerateMipChain(chain.data(), items, levels, px, mip_flags), "the mip chain");
        if (normal_ops & 4u) stage(itwPrepareNormalMapChain(chain.data(), items * levels, px, 4u), "the normalise");
        done = itwCompressImageChainEx(chain.data(), items * levels, target, dxgi_format, settings, progress, user);
        itw::chain_scratch_done(st);
    });
    return ok && done;
}

} // namespace

extern "C" bool itwCompressImageMippedEx(const rgba_surface* bases, int items, int levels, uint32_t normal_ops, uint32_t mip_flags, uint8_t* target,
                                         int dxgi_format, const void* settings, ItwProgressFunc* progress, void* user)
{
    if (mip_flags & ITW_MIP_VOLUME) {                                     // a volume: `bases` are its `items` slices (mip3d.hip)
        if (normal_ops) {
            itw::clear_failure();
            itw::guarded([&] { itw::fail_msg("itwCompressImageMipped: normal ops 0x%x with ITW_MIP_VOLUME: a volume holds no normal map the stages know", normal_ops); });
            return false;
        }
        return itw::compress_volume_mipped("itwCompressImageMipped", bases, items, levels, mip_flags & ~(uint32_t)ITW_MIP_VOLUME, target, dxgi_format, settings, progress, user);
    }
    return compress_mipped(bases, items, levels, normal_ops, mip_flags, false, nullptr, target, dxgi_format, settings, progress, user);
}

extern "C" bool itwCompressImageMippedAlpha(const rgba_surface* bases, int items, int levels, uint32_t mip_flags, const itw_mip_alpha* alpha, uint8_t* target,
                                            int dxgi_format, const void* settings, ItwProgressFunc* progress, void* user)
{
    return compress_mipped(bases, items, levels, 0, mip_flags, true, alpha, target, dxgi_format, settings, progress, user);
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
        itw::check_normal_ops("itwCompressSignedNormalMapMipped", ops);
        itw::chain_check_with(bases, items, target, dxgi_format, nullptr);        // counts, null pointers, sizes, format
        const MippedBases b = check_mipped_bases("itwCompressSignedNormalMapMipped", bases, items, levels, texel_bytes, 8);
        const int w = bases[0].width, h = bases[0].height;
        levels = b.levels;

        // the thread's chain buffer: [RGBA16F chain] [host bases as they are]
        hipStream_t st = (hipStream_t)itwGetStream();
        const itw::StagingPlan plan(bases, items, texel_bytes, b.dev, (size_t)b.chain_bytes);
        uint8_t* buf = static_cast<uint8_t*>(itw::chain_scratch(plan.bytes, st));
        std::vector<rgba_surface> chain((size_t)items * levels);
        itwMipChainLayout(w, h, items, levels, 8, buf, chain.data());
        const int64_t quads = itw::texel_quads(w, h);                             // (within one launch: check_launch_limits bounds the tiles of 64 x 64)
        if (!itw::quads_fit_one_launch(quads)) itw::fail_msg("itwCompressSignedNormalMapMipped: a %d x %d base is more than one launch covers", w, h);
        const dim3 grid((unsigned)((quads + 255) / 256)), blk(256);
        for (int i = 0; i < items; i++) {
            itw::upload_image(plan, buf, i, st);
            const uint8_t* src = plan.ptr(i, buf);
            const int64_t stride = plan.stride(i);
            const rgba_surface& l0 = chain[(size_t)i * levels];
            if (ops & ITW_NORMAL_FROM_HEIGHT) {                                   // the bases are height maps: differenced at their own precision
                itw::height_level0(itw::height_signed_source_kind(texel_bytes), itw::hn::DST_HALF_SIGNED, src, stride, l0, ops & ~4u, st);
                continue;
            }
            if (texel_bytes == 4)      hipLaunchKernelGGL((itw::mip_widen_signed_kernel<4>), grid, blk, 0, st, src, stride, l0.ptr, (int64_t)l0.stride, w, h, ops & 3u);
            else if (texel_bytes == 8) hipLaunchKernelGGL((itw::mip_widen_signed_kernel<8>), grid, blk, 0, st, src, stride, l0.ptr, (int64_t)l0.stride, w, h, ops & 3u);
            else                       hipLaunchKernelGGL((itw::mip_widen_signed_kernel<16>), grid, blk, 0, st, src, stride, l0.ptr, (int64_t)l0.stride, w, h, ops & 3u);
            ITW_CHECK(hipGetLastError());
        }
        if (itwGenerateMipChain(chain.data(), items, levels, 8, 0) != 0) itw::fail_msg("itwCompressSignedNormalMapMipped: the mip chain failed: %s", itwLastError());
        // the normalise runs in fp32 on every level inside the chain's gather: no pass of its own, no rounding to half before the quantisation
        done = itwCompressSignedNormalMapChain(chain.data(), items * levels, 8, target, dxgi_format, ops & 4u, progress, user);
        itw::chain_scratch_done(st);
    });
    return ok && done;
}
