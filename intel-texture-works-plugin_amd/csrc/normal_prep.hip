// normal_prep.hip -- the normal-map stages of the reference's save path as a pre-pass of their own (include/itw_dispatch.h:
// itwPrepareNormalMapChain; IntelPlugin.cpp:2103-2106 FlipXYChannelNormalMap, :2149-2152 NormalizeNormalMapChain), and the cube-cross
// views (itwCubeCrossFaces; :1200-1265 ConvertToCubeMapFromCross).  The arithmetic is normal_prep.hpp's.
//
// Every image of a chain in ONE launch, in place: a lane takes four consecutive texels of one row (a "quad": 16 B of RGBA8, 32 B of
// RGBA16F), lane = quad of the chain's concatenated quad list, its image found by binary search over a small level table as
// decode_chain_kernel finds its (a chain of one travels as a kernel argument).  A whole quad at a 16-byte address moves as dwordx4, anything
// else texel by texel, so a pointer or stride that is only texel aligned works and nothing outside width x height is read or written.
// A stream: HBM bound.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>
#include "../../include/itw_dispatch.h"
#include "../../include/itw_amd.h"
#include "normal_prep.hpp"
#include "host_rt.hpp"
#include "kernels.hpp"

namespace itw {

// one image: texels at `ptr`, rows `stride` bytes apart, and the index of its first quad in the chain's list (ceil(width / 4) * height each)
struct PrepLevel { uint8_t* ptr; int64_t stride; int32_t width, height; int64_t first_quad; };

template <int PX>
__device__ __forceinline__ void normal_prep_quad(const PrepLevel& lv, int64_t q, uint32_t ops)
{
    const int32_t qpr = (lv.width + 3) >> 2;
    int64_t y;
    int32_t qx;
    if (q < ((int64_t)1 << 31)) { const uint32_t yy = (uint32_t)q / (uint32_t)qpr; y = yy; qx = (int32_t)((uint32_t)q - yy * (uint32_t)qpr); }
    else                        { y = q / qpr; qx = (int32_t)(q - y * qpr); }
    const int32_t n = min(4, lv.width - 4 * qx);                  // texels of this quad inside the row
    uint8_t* p = lv.ptr + y * lv.stride + (int64_t)qx * 4 * PX;
    if (n == 4 && ((uintptr_t)p & 15) == 0) {
        uint4* p4 = reinterpret_cast<uint4*>(p);
        if (PX == 4) {
            uint4 t = p4[0];
            t.x = normal_prep_rgba8(t.x, ops); t.y = normal_prep_rgba8(t.y, ops); t.z = normal_prep_rgba8(t.z, ops); t.w = normal_prep_rgba8(t.w, ops);
            p4[0] = t;
        } else {
            uint4 a = p4[0], b = p4[1];
            normal_prep_rgba16f(a.x, a.y, ops); normal_prep_rgba16f(a.z, a.w, ops);
            normal_prep_rgba16f(b.x, b.y, ops); normal_prep_rgba16f(b.z, b.w, ops);
            p4[0] = a; p4[1] = b;
        }
    } else {
        uint32_t* p1 = reinterpret_cast<uint32_t*>(p);            // texel aligned: 4 bytes (RGBA8), 8 bytes (RGBA16F)
        for (int x = 0; x < n; x++) {
            if (PX == 4) p1[x] = normal_prep_rgba8(p1[x], ops);
            else { uint32_t lo = p1[2 * x], hi = p1[2 * x + 1]; normal_prep_rgba16f(lo, hi, ops); p1[2 * x] = lo; p1[2 * x + 1] = hi; }
        }
    }
}

// ONE: a chain of one image; its descriptor is the kernel argument `one` and there is no table and no search
template <int PX, bool ONE>
__global__ void __launch_bounds__(256)
normal_prep_kernel(const PrepLevel* __restrict__ levels, const PrepLevel one, int32_t nlev, int64_t nquads, uint32_t ops)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nquads) return;
    if (ONE) { normal_prep_quad<PX>(one, j, ops); return; }
    int lo = 0, hi = nlev - 1;                                    // the last image whose first quad is <= j
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (levels[mid].first_quad <= j) lo = mid; else hi = mid - 1;
    }
    const PrepLevel lv = levels[lo];
    normal_prep_quad<PX>(lv, j - lv.first_quad, ops);
}

// ---- itwQuantizeNormalMapChain: signed normal sources (normal_prep.hpp) to RGBA8_SNORM, out of place -----------------------------------------
// The same walk: a lane takes a quad of one row of one image, 4 * TB source bytes into 16 target bytes.  A target may be its own source when
// TB == 4: a lane reads its quad before it writes it and no other lane touches those texels.
struct QuantLevel { const uint8_t* src; uint8_t* dst; int64_t src_stride, dst_stride; int32_t width, height; int64_t first_quad; };

template <int TB>
__device__ __forceinline__ void normal_quantize_quad(const QuantLevel& lv, int64_t q, uint32_t ops)
{
    const int32_t qpr = (lv.width + 3) >> 2;
    int64_t y;
    int32_t qx;
    if (q < ((int64_t)1 << 31)) { const uint32_t yy = (uint32_t)q / (uint32_t)qpr; y = yy; qx = (int32_t)((uint32_t)q - yy * (uint32_t)qpr); }
    else                        { y = q / qpr; qx = (int32_t)(q - y * qpr); }
    const int32_t n = min(4, lv.width - 4 * qx);                  // texels of this quad inside the row
    const uint8_t* s = lv.src + y * lv.src_stride + (int64_t)qx * 4 * TB;
    uint8_t* d = lv.dst + y * lv.dst_stride + (int64_t)qx * 16;
    constexpr int WPT = TB / 4;                                   // words per source texel
    uint32_t w[4 * WPT], o[4];
    const bool vec_in = n == 4 && ((uintptr_t)s & 15) == 0;
    if (vec_in) {
        const uint4* s4 = reinterpret_cast<const uint4*>(s);
#pragma unroll
        for (int k = 0; k < WPT; k++) { const uint4 t = s4[k]; w[4 * k] = t.x; w[4 * k + 1] = t.y; w[4 * k + 2] = t.z; w[4 * k + 3] = t.w; }
    } else {
        const uint32_t* s1 = reinterpret_cast<const uint32_t*>(s);    // texel aligned, so word aligned
#pragma unroll
        for (int k = 0; k < 4 * WPT; k++) w[k] = k < n * WPT ? s1[k] : 0u;
    }
#pragma unroll
    for (int x = 0; x < 4; x++) {
        float v[4];
        normal_load_signed<TB>(v, w + x * WPT);
        o[x] = normal_quantize_texel(v, ops);
    }
    if (n == 4 && ((uintptr_t)d & 15) == 0) *reinterpret_cast<uint4*>(d) = make_uint4(o[0], o[1], o[2], o[3]);
    else {
        uint32_t* d1 = reinterpret_cast<uint32_t*>(d);
#pragma unroll
        for (int x = 0; x < 4; x++) if (x < n) d1[x] = o[x];
    }
}

template <int TB, bool ONE>
__global__ void __launch_bounds__(256)
normal_quantize_kernel(const QuantLevel* __restrict__ levels, const QuantLevel one, int32_t nlev, int64_t nquads, uint32_t ops)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nquads) return;
    if (ONE) { normal_quantize_quad<TB>(one, j, ops); return; }
    int lo = 0, hi = nlev - 1;                                    // the last image whose first quad is <= j
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (levels[mid].first_quad <= j) lo = mid; else hi = mid - 1;
    }
    const QuantLevel lv = levels[lo];
    normal_quantize_quad<TB>(lv, j - lv.first_quad, ops);
}

template <int TB>
void launch_normal_quantize(const QuantLevel* d_desc, const QuantLevel& first, int count, int64_t quads, uint32_t ops, hipStream_t st)
{
    const dim3 grid((unsigned)((quads + 255) / 256)), blk(256);
    if (count == 1) hipLaunchKernelGGL((normal_quantize_kernel<TB, true>), grid, blk, 0, st, d_desc, first, 1, quads, ops);
    else            hipLaunchKernelGGL((normal_quantize_kernel<TB, false>), grid, blk, 0, st, d_desc, first, (int32_t)count, quads, ops);
}

} // namespace itw

namespace {

// everything that needs the device: `count` >= 1 images that passed the checks, all of one pointer kind
void prepare_chain(const rgba_surface* im, int count, int px, uint32_t ops, bool dev)
{
    hipStream_t st = (hipStream_t)itwGetStream();
    static thread_local std::vector<itw::PrepLevel> desc;         // grow-only, like the device buffer it is copied into
    desc.resize((size_t)count);
    // the thread's buffer: [level table] [staged images (host pointers)]
    const itw::StagingPlan plan(im, count, px, dev, count > 1 ? (size_t)count * sizeof(itw::PrepLevel) : 0);
    int64_t quads = 0;
    for (int i = 0; i < count; i++) {
        desc[(size_t)i] = itw::PrepLevel{im[i].ptr, plan.stride(i), im[i].width, im[i].height, quads};
        quads += itw::texel_quads(im[i].width, im[i].height);
    }
    if (!itw::quads_fit_one_launch(quads)) itw::fail_msg("itwPrepareNormalMapChain: %lld texel quads are more than one launch covers", (long long)quads);
    const bool buffer = !dev || count > 1;                        // a resident chain of one touches no buffer of the thread
    uint8_t* base = buffer ? static_cast<uint8_t*>(itw::decode_scratch(plan.bytes, st)) : nullptr;
    if (!dev) for (int i = 0; i < count; i++) desc[(size_t)i].ptr = plan.ptr(i, base);
    itw::upload_staged(plan, base, st);
    if (count > 1) ITW_CHECK(hipMemcpyAsync(base, desc.data(), (size_t)count * sizeof(itw::PrepLevel), hipMemcpyHostToDevice, st));
    const itw::PrepLevel* d_desc = count > 1 ? reinterpret_cast<const itw::PrepLevel*>(base) : nullptr;
    const dim3 grid((unsigned)((quads + 255) / 256)), blk(256);
    if (px == 4) {
        if (count == 1) hipLaunchKernelGGL((itw::normal_prep_kernel<4, true>), grid, blk, 0, st, d_desc, desc[0], 1, quads, ops);
        else            hipLaunchKernelGGL((itw::normal_prep_kernel<4, false>), grid, blk, 0, st, d_desc, desc[0], (int32_t)count, quads, ops);
    } else {
        if (count == 1) hipLaunchKernelGGL((itw::normal_prep_kernel<8, true>), grid, blk, 0, st, d_desc, desc[0], 1, quads, ops);
        else            hipLaunchKernelGGL((itw::normal_prep_kernel<8, false>), grid, blk, 0, st, d_desc, desc[0], (int32_t)count, quads, ops);
    }
    ITW_CHECK(hipGetLastError());
    if (dev) { if (buffer) itw::decode_scratch_done(st); return; }     // resident: asynchronous on the thread's stream
    itw::download_staged(plan, base, st);                         // width x height only: the caller's row padding is not written
    ITW_CHECK(hipStreamSynchronize(st));
    itw::decode_scratch_done(st);
}

// itwQuantizeNormalMapChain's device work: `count` >= 1 pairs that passed the checks, all of one pointer kind
void quantize_chain(const rgba_surface* src, int tb, const rgba_surface* dst, int count, uint32_t ops, bool dev)
{
    hipStream_t st = (hipStream_t)itwGetStream();
    static thread_local std::vector<itw::QuantLevel> desc;        // grow-only, like the device buffer it is copied into
    desc.resize((size_t)count);
    // the thread's buffer: [level table] [staged sources] [staged targets] (host pointers)
    const itw::StagingPlan from(src, count, tb, dev, count > 1 ? (size_t)count * sizeof(itw::QuantLevel) : 0), to(dst, count, 4, dev, from.bytes);
    int64_t quads = 0;
    for (int i = 0; i < count; i++) {
        desc[(size_t)i] = itw::QuantLevel{src[i].ptr, dst[i].ptr, from.stride(i), to.stride(i), src[i].width, src[i].height, quads};
        quads += itw::texel_quads(src[i].width, src[i].height);
    }
    if (!itw::quads_fit_one_launch(quads)) itw::fail_msg("itwQuantizeNormalMapChain: %lld texel quads are more than one launch covers", (long long)quads);
    const bool buffer = !dev || count > 1;                        // a resident chain of one touches no buffer of the thread
    uint8_t* base = buffer ? static_cast<uint8_t*>(itw::decode_scratch(to.bytes, st)) : nullptr;
    if (!dev) for (int i = 0; i < count; i++) { desc[(size_t)i].src = from.ptr(i, base); desc[(size_t)i].dst = to.ptr(i, base); }
    itw::upload_staged(from, base, st);
    if (count > 1) ITW_CHECK(hipMemcpyAsync(base, desc.data(), (size_t)count * sizeof(itw::QuantLevel), hipMemcpyHostToDevice, st));
    const itw::QuantLevel* d_desc = count > 1 ? reinterpret_cast<const itw::QuantLevel*>(base) : nullptr;
    if (tb == 4)      itw::launch_normal_quantize<4>(d_desc, desc[0], count, quads, ops, st);
    else if (tb == 8) itw::launch_normal_quantize<8>(d_desc, desc[0], count, quads, ops, st);
    else              itw::launch_normal_quantize<16>(d_desc, desc[0], count, quads, ops, st);
    ITW_CHECK(hipGetLastError());
    if (dev) { if (buffer) itw::decode_scratch_done(st); return; }     // resident: asynchronous on the thread's stream
    itw::download_staged(to, base, st);                           // width x height only: the caller's row padding is not written
    ITW_CHECK(hipStreamSynchronize(st));
    itw::decode_scratch_done(st);
}

} // namespace

extern "C" int itwQuantizeNormalMapChain(const rgba_surface* sources, int texel_bytes, const rgba_surface* targets, int count, uint32_t ops)
{
    itw::clear_failure();
    bool dev = false;
    // the refusals: through the error mode, before any device work
    const bool ok = itw::guarded([&] {
        if (count < 0) itw::fail_msg("itwQuantizeNormalMapChain: count %d", count);
        if (texel_bytes != 4 && texel_bytes != 8 && texel_bytes != 16) itw::fail_msg("itwQuantizeNormalMapChain: texel_bytes %d (4, 8 or 16)", texel_bytes);
        itw::check_normal_ops("itwQuantizeNormalMapChain", ops);
        if (count == 0) return;
        if (!sources || !targets) itw::fail_msg("itwQuantizeNormalMapChain: null image list");
        itw::check_images("itwQuantizeNormalMapChain", "source", sources, count, texel_bytes, texel_bytes);
        for (int i = 0; i < count; i++) {
            const rgba_surface& s = sources[i];
            const rgba_surface& t = targets[i];
            if (t.width != s.width || t.height != s.height)
                itw::fail_msg("itwQuantizeNormalMapChain: image %d: the target is %d x %d, its source %d x %d", i, t.width, t.height, s.width, s.height);
        }
        itw::check_images("itwQuantizeNormalMapChain", "target", targets, count, 4, 4);
        if (ops & ITW_NORMAL_FROM_HEIGHT) itw::height_check_disjoint("itwQuantizeNormalMapChain", sources, texel_bytes, targets, count);
    });
    if (!ok) return -1;
    if (count == 0) return 0;
    const bool done = itw::guarded([&] {
        dev = itw::all_one_pointer_kind("itwQuantizeNormalMapChain", "image", sources, count, targets);
        if (ops & ITW_NORMAL_FROM_HEIGHT) itw::height_quantize_chain(sources, texel_bytes, targets, count, ops, dev);
        else                              quantize_chain(sources, texel_bytes, targets, count, ops, dev);
    });
    return done ? 0 : -1;
}

extern "C" int itwPrepareNormalMapChain(const rgba_surface* images, int count, int pixel_size, uint32_t ops)
{
    if (count < 0 || (pixel_size != 4 && pixel_size != 8) || itw::normal_ops_fault(ops)) return -1;
    if (count == 0) return 0;
    if (!images) return -1;
    if (itw::image_list_fault(images, count, pixel_size, pixel_size)) return -1;         // silently, like the rest: never through the error mode
    if (ops == 0) return 0;
    const bool dev = itw::is_device_pointer(images[0].ptr);
    for (int i = 1; i < count; i++)
        if (itw::is_device_pointer(images[i].ptr) != dev) return -1;     // all host or all device, as the chain encoder asks
    const bool ok = itw::guarded([&] {
        if (ops & ITW_NORMAL_FROM_HEIGHT) itw::height_prepare_chain(images, count, pixel_size, ops, dev);     // every image a height map on entry
        else                              prepare_chain(images, count, pixel_size, ops, dev);
    });
    return ok ? 0 : -1;
}

// IntelPlugin.cpp:1206-1233: the six rectangles of a horizontal (4 x 3 cells) or vertical (3 x 4) cross, +X -X +Y -Y +Z -Z; cell sizes are
// truncating quotients, exactly as the reference's.  Views: no rotation and no copy (its CopyRectangle calls copy the rectangles as they lie)
extern "C" int itwCubeCrossFaces(const rgba_surface* cross, int pixel_size, rgba_surface faces[6])
{
    if (!cross || !faces || !cross->ptr || (pixel_size != 4 && pixel_size != 8 && pixel_size != 16)) return -1;
    int cells[6][2] = {{2, 1}, {0, 1}, {1, 0}, {1, 2}, {1, 1}, {3, 1}};
    const bool vertical = cross->width < cross->height;
    if (cross->width < (vertical ? 3 : 4) || cross->height < (vertical ? 4 : 3)) return -1;
    const int32_t w = cross->width / (vertical ? 3 : 4), h = cross->height / (vertical ? 4 : 3);
    if (vertical) { cells[5][0] = 1; cells[5][1] = 3; }
    for (int i = 0; i < 6; i++) {
        faces[i].ptr = cross->ptr + (int64_t)cells[i][1] * h * cross->stride + (int64_t)cells[i][0] * w * pixel_size;
        faces[i].width = w; faces[i].height = h; faces[i].stride = cross->stride;
    }
    return 0;
}
