// mip3d.hip -- the mip chain of a volume texture, GenerateMipMaps3D (DirectXTexMipmaps.cpp:2884-2983) on the device: DirectXTex's five 3D
// filters behind ITW_MIP_VOLUME (include/itw_dispatch.h, "Mip chains: volumes"; the kernels are mip3d_kernels.hpp's; mipgen.hip's entry points hand over), and the volume save path in one call
// (itwCompressImageMippedEx with ITW_MIP_VOLUME).  A chain is a list of slices in DDS volume order, level-major; level l is filtered from the STORED level l-1,
// one launch per level.  The entry point's checks, staging and upload follow mipgen.hip's generate_checked / generate_chain: one upload
// carries the image table and, for the triangle filter, the gather lists of every level and all three axes behind it.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../include/itw_dispatch.h"
#include "../../include/itw_amd.h"
#include "mipgen.hpp"
#include "mip_kernels.hpp"
#include "mip_filters.hpp"
#include "mip3d_kernels.hpp"
#include "mip3d.hpp"
#include "bcn_format.hpp"
#include "host_rt.hpp"

namespace {

using itw::mip_dim;

constexpr int kMaxLevels = 32;

// a call's filter as its checks left it: kind is a MipFilterKind, never MIP_FILTER_DEFAULT once the sizes are known
struct Filter3d { int kind = 0; bool wrap_u = false, wrap_v = false, wrap_w = false; };

constexpr uint32_t kFilterBits = ITW_MIP_POINT | ITW_MIP_LINEAR | ITW_MIP_CUBIC | ITW_MIP_TRIANGLE;
constexpr uint32_t kFlags3d = ITW_MIP_PER_LEVEL | ITW_MIP_SRGB | kFilterBits | ITW_MIP_WRAP_U | ITW_MIP_WRAP_V | ITW_MIP_WRAP_W;

// the flag bits of a 3D call; `what` is "flag" or "mip flag" as the entry point's messages have it
Filter3d check_flags(const char* who, const char* what, uint32_t flags)
{
    if (flags & ITW_MIP_RESIZE) itw::fail_msg("%s: ITW_MIP_RESIZE: a volume chain has the definition's sizes (DirectXTex has no 3D resize)", who);
    if (flags & (ITW_MIP_MIRROR_U | ITW_MIP_MIRROR_V)) itw::fail_msg("%s: ITW_MIP_MIRROR_U / _V are the free-size chain's: at a volume chain's ratios mirror is clamp", who);
    if (flags & ~kFlags3d) itw::fail_msg("%s: unknown %s bits 0x%x", who, what, flags & ~kFlags3d);
    const uint32_t named = flags & kFilterBits;
    if (named & (named - 1))
        itw::fail_msg("%s: two filter bits together (0x%x): a chain takes one of ITW_MIP_POINT, ITW_MIP_LINEAR, ITW_MIP_CUBIC and ITW_MIP_TRIANGLE", who, named);
    Filter3d f;
    f.kind = (flags & ITW_MIP_CUBIC) ? itw::MIP_FILTER_CUBIC : (flags & ITW_MIP_TRIANGLE) ? itw::MIP_FILTER_TRIANGLE
           : (flags & ITW_MIP_POINT) ? itw::MIP_FILTER_POINT : (flags & ITW_MIP_LINEAR) ? itw::MIP_FILTER_LINEAR : itw::MIP_FILTER_DEFAULT;
    f.wrap_u = (flags & ITW_MIP_WRAP_U) != 0; f.wrap_v = (flags & ITW_MIP_WRAP_V) != 0; f.wrap_w = (flags & ITW_MIP_WRAP_W) != 0;
    return f;
}

// GenerateMipMaps3D's default (:2921-2926): box when all three sizes are powers of two, triangle otherwise
int resolve_default(int kind, int w, int h, int d)
{
    if (kind != itw::MIP_FILTER_DEFAULT) return kind;
    return itw::mip_pow2(w) && itw::mip_pow2(h) && itw::mip_pow2(d) ? itw::MIP_FILTER_BOX : itw::MIP_FILTER_TRIANGLE;
}

// What one launch covers, checked before any device work: a plane of the grid per destination slice and a block row per 4 texel rows
// (65 535 each), over level 1, the largest written.
void check_launch_limits(const char* who, int h, int d)
{
    if (mip_dim(d, 1) > 65535) itw::fail_msg("%s: a base of %d slices is more than one launch covers (131 071)", who, d);
    if (mip_dim(h, 1) > 4 * 65535) itw::fail_msg("%s: a base of %d rows is more than one launch covers (524 280)", who, h);
}

// the triangle filter's gather lists of every level and the three axes: `words` travels behind the image table
struct TapPlan3d {
    std::vector<uint32_t> words, off;                                     // off[3 * l + axis]
    std::vector<int> built_for;
    size_t build(const Filter3d& f, int levels, int w, int h, int d)
    {
        if (f.kind != itw::MIP_FILTER_TRIANGLE) return 0;
        const std::vector<int> key = { f.wrap_u, f.wrap_v, f.wrap_w, levels, w, h, d };
        if (!words.empty() && key == built_for) return words.size() * sizeof(uint32_t);
        built_for.clear();
        words.clear(); off.assign((size_t)levels * 3, 0u);
        std::vector<itw::MipTriEntry> lists;
        for (int l = 1; l < levels; l++)
            for (int axis = 0; axis < 3; axis++) {
                const int base = axis == 0 ? w : axis == 1 ? h : d;
                const int source = mip_dim(base, l - 1), dest = mip_dim(base, l);
                itw::mip_triangle_lists(source, dest, axis == 0 ? f.wrap_u : axis == 1 ? f.wrap_v : f.wrap_w, lists);
                if ((words.size() + (size_t)dest + 1) & 1u) words.push_back(0u);          // the entries, two words each, start on 8 bytes
                if (words.size() + (size_t)dest + 1 + 2 * lists.size() > (size_t)0x7fffffff)
                    itw::fail_msg("volume mip chain: the triangle filter's lists of a %d x %d x %d base are more than a launch addresses", w, h, d);
                off[(size_t)l * 3 + axis] = (uint32_t)words.size();
                bool twice = false;                                       // (the kernel groups a source's entries whether or not one repeats)
                if (!itw::mip_triangle_gather(lists, dest, words, &twice))
                    itw::fail_msg("volume mip chain: the triangle filter's lists of %d -> %d name a destination outside the level", source, dest);
            }
        built_for = key;
        return words.size() * sizeof(uint32_t);
    }
};

template <int PX, bool SRGB>
void launch_levels(const itw::MipImage* table, const uint32_t* taps, const TapPlan3d& plan, const Filter3d& f, int levels, int w, int h, int d, hipStream_t st)
{
    int first = 0;                                                        // of level l - 1 in the table
    for (int l = 1; l < levels; l++) {
        itw::Mip3dLevel lv;
        lv.sw = mip_dim(w, l - 1); lv.sh = mip_dim(h, l - 1); lv.sd = mip_dim(d, l - 1);
        lv.ow = mip_dim(w, l); lv.oh = mip_dim(h, l); lv.od = mip_dim(d, l);
        lv.src_first = first; lv.dst_first = first + lv.sd;
        first += lv.sd;
        const dim3 grid((unsigned)((lv.ow + 63) / 64), (unsigned)((lv.oh + 3) / 4), (unsigned)lv.od), blk(256);
        const float scale_x = (float)lv.sw / (float)lv.ow, scale_y = (float)lv.sh / (float)lv.oh, scale_z = (float)lv.sd / (float)lv.od;
        const uint32_t wrap = (f.wrap_u ? 1u : 0u) | (f.wrap_v ? 2u : 0u) | (f.wrap_w ? 4u : 0u);
        switch (f.kind) {
        case itw::MIP_FILTER_BOX:    hipLaunchKernelGGL((itw::mip3d_box_kernel<PX, SRGB>), grid, blk, 0, st, table, lv); break;
        case itw::MIP_FILTER_POINT:  hipLaunchKernelGGL((itw::mip3d_point_kernel<PX, SRGB>), grid, blk, 0, st, table, lv); break;
        case itw::MIP_FILTER_LINEAR: hipLaunchKernelGGL((itw::mip3d_linear_kernel<PX, SRGB>), grid, blk, 0, st, table, lv, scale_x, scale_y, scale_z); break;
        case itw::MIP_FILTER_CUBIC:  hipLaunchKernelGGL((itw::mip3d_cubic_kernel<PX, SRGB>), grid, blk, 0, st, table, lv, scale_x, scale_y, scale_z, wrap); break;
        default:
            hipLaunchKernelGGL((itw::mip3d_triangle_kernel<PX, SRGB>), grid, blk, 0, st, table, lv, taps, plan.off[(size_t)l * 3], plan.off[(size_t)l * 3 + 1],
                               plan.off[(size_t)l * 3 + 2]);
        }
        ITW_CHECK(hipGetLastError());
    }
}

// everything that needs the device: a slice list that passed the checks, all of one pointer kind, levels >= 2
void generate_volume(const rgba_surface* im, int count, int depth, int levels, int px, bool srgb, bool dev, const Filter3d& filter)
{
    hipStream_t st = (hipStream_t)itwGetStream();
    const int w = im[0].width, h = im[0].height;
    // what one upload carries: the image table, then the triangle filter's lists 256-B aligned behind it
    static thread_local std::vector<uint8_t> head;                        // grow-only, like the device buffer it is copied into
    static thread_local TapPlan3d taps;
    const size_t table_bytes = (size_t)count * sizeof(itw::MipImage), taps_off = itw::up256(table_bytes);
    const size_t taps_bytes = taps.build(filter, levels, w, h, depth), head_bytes = taps_bytes ? taps_off + taps_bytes : table_bytes;
    head.resize(head_bytes);
    if (taps_bytes) std::memcpy(head.data() + taps_off, taps.words.data(), taps_bytes);
    itw::MipImage* desc = reinterpret_cast<itw::MipImage*>(head.data());
    const itw::StagingPlan plan(im, count, px, dev, head_bytes);         // the thread's buffer: [table, lists] [staged slices (host pointers)]
    uint8_t* base = static_cast<uint8_t*>(itw::decode_scratch(plan.bytes, st));
    for (int i = 0; i < count; i++) desc[i] = itw::MipImage{plan.ptr(i, base), plan.stride(i)};
    for (int i = 0; i < depth; i++) itw::upload_image(plan, base, i, st);                                             // only level 0 goes up
    ITW_CHECK(hipMemcpyAsync(base, head.data(), head_bytes, hipMemcpyHostToDevice, st));
    const itw::MipImage* table = reinterpret_cast<const itw::MipImage*>(base);
    const uint32_t* lists = reinterpret_cast<const uint32_t*>(base + taps_off);
    if (srgb)         launch_levels<4, true>(table, lists, taps, filter, levels, w, h, depth, st);                    // (the entry point refused it with px 8)
    else if (px == 4) launch_levels<4, false>(table, lists, taps, filter, levels, w, h, depth, st);
    else              launch_levels<8, false>(table, lists, taps, filter, levels, w, h, depth, st);
    if (!dev) {
        for (int i = depth; i < count; i++) itw::download_image(plan, base, i, st);                                   // only the written levels come back
        ITW_CHECK(hipStreamSynchronize(st));
    }
    itw::decode_scratch_done(st);
}

} // namespace

namespace itw {

int mip_levels_3d(int width, int height, int depth)
{
    if (width < 1 || height < 1 || depth < 1) return 0;
    int n = 1;
    for (int m = std::max(width, std::max(height, depth)); m > 1; m >>= 1) n++;
    return n;
}

int mip_slices_3d(int depth, int levels)
{
    if (depth < 1 || levels < 0 || levels > kMaxLevels) return -1;
    int64_t n = 0;
    for (int l = 0; l < levels; l++) n += mip_dim(depth, l);
    return n > (int64_t)0x7fffffff ? -1 : (int)n;
}

int64_t mip_chain_layout_3d(int width, int height, int depth, int levels, int pixel_size, uint8_t* storage, rgba_surface* out)
{
    const int full = mip_levels_3d(width, height, depth);
    if (full == 0 || levels < 0 || levels > full || (pixel_size != 4 && pixel_size != 8)) return -1;
    if ((int64_t)width * pixel_size > (int64_t)0x7fffffff) return -1;     // rgba_surface's stride is an int32
    if (levels == 0) levels = full;
    int64_t off = 0;
    size_t i = 0;
    for (int l = 0; l < levels; l++) {
        const int w = mip_dim(width, l), h = mip_dim(height, l), d = mip_dim(depth, l);
        for (int z = 0; z < d; z++, i++) {
            if (out) {
                rgba_surface& s = out[i];
                s.ptr = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(storage) + (uintptr_t)off);
                s.width = w; s.height = h; s.stride = w * pixel_size;
            }
            off += (int64_t)w * h * pixel_size;
        }
    }
    return off;
}

int generate_mip_chain_3d(const char* who, const rgba_surface* slices, int depth, int levels, int pixel_size, uint32_t flags)
{
    itw::clear_failure();
    const bool ok = itw::guarded([&] {
        if (pixel_size != 4 && pixel_size != 8) itw::fail_msg("%s: pixel_size %d (4: RGBA8, 8: RGBA16F)", who, pixel_size);
        Filter3d filter = check_flags(who, "flag", flags);
        if ((flags & ITW_MIP_SRGB) && pixel_size != 4) itw::fail_msg("%s: ITW_MIP_SRGB is for RGBA8 texels (pixel_size 4): RGBA16F is linear already", who);
        if (depth < 0) itw::fail_msg("%s: depth %d", who, depth);
        if (depth == 0 || levels <= 1) return;
        if (!slices) itw::fail_msg("%s: null slices pointer", who);
        const int w = slices[0].width, h = slices[0].height, full = mip_levels_3d(w, h, depth);
        if (full == 0) itw::fail_msg("%s: the base is %d x %d x %d", who, w, h, depth);
        if (levels > full) itw::fail_msg("%s: %d levels, a full chain of %d x %d x %d has %d", who, levels, w, h, depth, full);
        check_launch_limits(who, h, depth);
        const int count = mip_slices_3d(depth, levels);
        if (count < 0 || count > 0x7fffffff / 64) itw::fail_msg("%s: %d levels of a depth of %d are more slices than one table holds", who, levels, depth);
        int i = 0;
        for (int l = 0; l < levels; l++)
            for (int z = 0; z < mip_dim(depth, l); z++, i++) {
                const rgba_surface& s = slices[i];
                const itw::ImageFaultKind fault = itw::image_fault(s, pixel_size, pixel_size);      // null texels come before the sizes, the rest after
                if (fault == itw::IMAGE_NULL_TEXELS) itw::fail_image(who, fault, s, pixel_size, pixel_size, "level %d slice %d", l, z);
                if (s.width != mip_dim(w, l) || s.height != mip_dim(h, l))
                    itw::fail_msg("%s: level %d slice %d is %d x %d, the chain's is %d x %d", who, l, z, s.width, s.height, mip_dim(w, l), mip_dim(h, l));
                if (fault) itw::fail_image(who, fault, s, pixel_size, pixel_size, "level %d slice %d", l, z);
            }
        const bool dev = itw::all_one_pointer_kind(who, "slice", slices, count);
        filter.kind = resolve_default(filter.kind, w, h, depth);
        generate_volume(slices, count, depth, levels, pixel_size, (flags & ITW_MIP_SRGB) != 0, dev, filter);
    });
    return ok ? 0 : -1;
}

bool compress_volume_mipped(const char* who, const rgba_surface* base_slices, int depth, int levels, uint32_t mip_flags, uint8_t* target, int dxgi_format,
                            const void* settings, ItwProgressFunc* progress, void* user)
{
    bool done = false;
    itw::clear_failure();
    const bool ok = itw::guarded([&] {
        itw::refuse_signed_bc6h(who, dxgi_format);
        check_flags(who, "mip flag", mip_flags);
        itw::chain_check_with(base_slices, depth, target, dxgi_format, settings);    // counts, null pointers, sizes, strides, format, settings
        const int px = itw::texel_bytes(itw::format_kind(dxgi_format));
        if (mip_flags & ITW_MIP_SRGB) {                                              // colour in RGBA8 codes, or nothing
            if (px != 4) itw::fail_msg("%s: ITW_MIP_SRGB with DXGI format %d, whose texels are RGBA16F: linear already", who, dxgi_format);
            if (dxgi_format == 81 || dxgi_format == 84) itw::fail_msg("%s: ITW_MIP_SRGB with DXGI format %d, whose texels are signed codes, not colour", who, dxgi_format);
        }
        const int w = base_slices[0].width, h = base_slices[0].height, full = mip_levels_3d(w, h, depth);
        for (int z = 0; z < depth; z++) {
            if (base_slices[z].width != w || base_slices[z].height != h)
                itw::fail_msg("%s: slice %d is %d x %d, slice 0 %d x %d", who, z, base_slices[z].width, base_slices[z].height, w, h);
            if (const itw::ImageFaultKind k = itw::image_fault(base_slices[z], px, px)) itw::fail_image(who, k, base_slices[z], px, px, "slice %d", z);
        }
        if (levels < 0 || levels > full) itw::fail_msg("%s: %d levels, a full chain of %d x %d x %d has %d", who, levels, w, h, depth, full);
        if (levels == 0) levels = full;
        check_launch_limits(who, h, depth);
        const int count = mip_slices_3d(depth, levels);
        if (count < 0 || count > 0x7fffffff / 64) itw::fail_msg("%s: %d levels of a depth of %d are more slices than one table holds", who, levels, depth);
        const bool dev = itw::all_one_pointer_kind(who, "slice", base_slices, depth);
        const int64_t bytes = mip_chain_layout_3d(w, h, depth, levels, px, nullptr, nullptr);
        if (bytes < 0) itw::fail_msg("%s: a %d x %d base is wider than a surface can describe", who, w, h);

        hipStream_t st = (hipStream_t)itwGetStream();
        std::vector<rgba_surface> chain((size_t)count);
        uint8_t* buf = static_cast<uint8_t*>(itw::chain_scratch((size_t)bytes, st));
        mip_chain_layout_3d(w, h, depth, levels, px, buf, chain.data());
        for (int z = 0; z < depth; z++)
            ITW_CHECK(hipMemcpy2DAsync(chain[(size_t)z].ptr, (size_t)chain[(size_t)z].stride, base_slices[z].ptr, (size_t)base_slices[z].stride, (size_t)w * px,
                                       (size_t)h, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        if (generate_mip_chain_3d(who, chain.data(), depth, levels, px, mip_flags) != 0) itw::fail_msg("%s: the mip chain failed: %s", who, itwLastError());
        done = itwCompressImageChainEx(chain.data(), count, target, dxgi_format, settings, progress, user);
        itw::chain_scratch_done(st);
    });
    return ok && done;
}

} // namespace itw
