// mip_alpha.hip -- the two rules of include/itw_dispatch.h ("Mip chains") for cut-out RGBA8 textures, on the device:
//   A. alpha-weighted colour.  The bodies of mip_kernels.hpp with WEIGHT = true, under names of their own (mipgen.o keeps exactly the
//      kernels it had): mip_alpha_pyramid_kernel<SRGB>, mip_alpha_tail_kernel<SRGB>, mip_alpha_level_kernel<LINEAR, SRGB>.  Same routes,
//      launches and LDS as the plain kinds; the filter call alone differs (mipgen.hpp mip_box_kind / mip_bilinear_kind).
//   B. coverage kept per level, three launches behind one another on the stream, each over every image of the call, no host read between:
//      mip_alpha_hist_kernel     a workgroup takes 16 384 texels of one image (a lane: four quads of a row at a time, 16 B each where
//                                the address allows).  Level 0: the count of texels with a >= ref, one global atomic per workgroup.  Levels >= 1: 256
//                                bins in LDS, one LDS atomic per texel, one global atomic per non-empty bin.  (A second instantiation
//                                counts the 0 and 255 bins per wave instead; it measured slower and only the hooks build launches it.)
//      mip_alpha_select_kernel   a workgroup per (item, level >= 1): ge[t], the target K, t* by a 64-bit packed lexicographic minimum,
//                                the table a -> a', the report rows.
//      mip_alpha_rescale_kernel  the hist kernel's walk over every level >= 1: the alpha byte through the level's table (LDS), 16 B
//                                loads and stores; a level whose t* is ref is left without a store.
//   Every count is an integer sum, so the order the atomics arrive in changes no bit.
// itwAlphaCoverage is the hist kernel's count path over an arbitrary list of images.
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
#include "mip_kernels.hpp"

namespace itw {

template <bool SRGB>
__global__ void __launch_bounds__(256)
mip_alpha_pyramid_kernel(const MipImage* __restrict__ table, int32_t levels, int32_t src_level, int32_t nout, int32_t tiles_x, int32_t tiles_per_item)
{
    mip_pyramid_body<4, SRGB, true>(table, levels, src_level, nout, tiles_x, tiles_per_item);
}

template <bool SRGB>
__global__ void __launch_bounds__(256)
mip_alpha_tail_kernel(const MipImage* __restrict__ table, int32_t levels, int32_t src_level, int32_t nout, int32_t w, int32_t h)
{
    mip_tail_body<4, SRGB, true>(table, levels, src_level, nout, w, h);
}

template <bool LINEAR, bool SRGB>
__global__ void __launch_bounds__(256)
mip_alpha_level_kernel(const MipImage* __restrict__ table, int32_t levels, int32_t dst_level, int32_t sw, int32_t sh, int32_t ow, int32_t oh,
                       float scale_x, float scale_y)
{
    mip_level_body<4, LINEAR, SRGB, true>(table, levels, dst_level, sw, sh, ow, oh, scale_x, scale_y);
}

void launch_chain_weighted(const MipImage* table, int items, int levels, int w, int h, bool srgb, bool per_level, hipStream_t st)
{
    static const MipKernels plain = { mip_alpha_pyramid_kernel<false>, mip_alpha_tail_kernel<false>, mip_alpha_level_kernel<false, false>,
                                      mip_alpha_level_kernel<true, false> };
    static const MipKernels light = { mip_alpha_pyramid_kernel<true>, mip_alpha_tail_kernel<true>, mip_alpha_level_kernel<false, true>,
                                      mip_alpha_level_kernel<true, true> };
    launch_chain(srgb ? light : plain, table, items, levels, w, h, per_level, st);
}

// ---- coverage ---------------------------------------------------------------------------------------------------------------------------

// One RGBA8 image of a coverage pass.  A workgroup walks 4096 quads (four texels of one row; the last quad of a row may be short) of one
// image; `first` is the image's first workgroup in the histogram launch, `first_rescale` in the rescale launch (level 0 has none there).
struct AlphaImage { uint8_t* ptr; int64_t stride; int32_t w, h; uint32_t first, first_rescale; };
static_assert(sizeof(AlphaImage) == 32, "the table is uploaded as it is");
constexpr int kAlphaPasses = 4;                                           // a lane takes four quads at a stride of 256, this many times
constexpr int kAlphaQuads = 256 * 4 * kAlphaPasses;                       // per workgroup

inline uint32_t alpha_blocks(int w, int h) { return (uint32_t)(((int64_t)((w + 3) >> 2) * h + kAlphaQuads - 1) / kAlphaQuads); }

// the image workgroup `b` belongs to: the last i whose first workgroup (RESCALE: first_rescale) is not above b.  Images without workgroups
// share their successor's number and are passed over.
template <bool RESCALE>
__device__ __forceinline__ int32_t alpha_image_of(const AlphaImage* __restrict__ table, int32_t count, uint32_t b)
{
    int32_t lo = 0, hi = count - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if ((RESCALE ? table[mid].first_rescale : table[mid].first) <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// quad `u` of `im` (u < quads of the image, or n = 0): its address, its texel count, and whether it is one 16-byte access
struct AlphaQuad { uint8_t* p; int32_t n; bool vec; };
__device__ __forceinline__ AlphaQuad alpha_quad(const AlphaImage& im, int64_t u, int64_t quads)
{
    AlphaQuad q;
    q.p = nullptr; q.n = 0; q.vec = false;
    if (u < quads) {
        const int32_t qpr = (im.w + 3) >> 2;
        const int32_t y = (int32_t)(u / qpr), qx = (int32_t)(u - (int64_t)y * qpr);
        q.p = im.ptr + (int64_t)y * im.stride + (int64_t)qx * 16;
        q.n = min(4, im.w - 4 * qx);
        q.vec = q.n == 4 && ((uintptr_t)q.p & 15) == 0;
    }
    return q;
}

__device__ __forceinline__ void alpha_quad_load(const AlphaQuad& q, uint32_t* w)
{
    if (q.vec) {
        const uint4 v = *reinterpret_cast<const uint4*>(q.p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) w[j] = j < q.n ? reinterpret_cast<const uint32_t*>(q.p)[j] : 0u;
    }
}

// `levels`: image i of the table is a level 0 when i % levels == 0 (itwAlphaCoverage: levels == 1, every image).  Level 0 adds its count
// of a >= ref to counts[i / levels]; any other level adds its histogram to hist[i * 256 ..].
// SPIKES: the 0 and 255 bins are counted per wave (ballot + popcount) and reach LDS once per wave -- cut-out alpha is two spikes there, and
// an LDS atomic per texel serialises on those two addresses.  false, the product's: one LDS atomic per texel, every bin.
template <bool SPIKES>
__global__ void __launch_bounds__(256)
mip_alpha_hist_kernel(const AlphaImage* __restrict__ table, int32_t count, int32_t levels, uint32_t ref, unsigned long long* __restrict__ counts,
                      unsigned long long* __restrict__ hist)
{
    __shared__ uint32_t bins[256];
    const int32_t img = alpha_image_of<false>(table, count, blockIdx.x);
    const AlphaImage im = table[img];
    const bool level0 = img % levels == 0;                                // (the workgroup's: no divergence below)
    const int64_t quads = (int64_t)((im.w + 3) >> 2) * im.h;
    const int64_t base = (int64_t)(blockIdx.x - im.first) * kAlphaQuads + threadIdx.x;
    bins[threadIdx.x] = 0;
    __syncthreads();
    uint32_t wave_lo = 0, wave_hi = 0;                                    // wave-wide counts: a >= ref (level 0), or a == 0 and a == 255
#pragma unroll 4
    for (int k = 0; k < 4 * kAlphaPasses; k++) {
        const AlphaQuad q = alpha_quad(im, base + k * 256, quads);
        uint32_t w[4];
        alpha_quad_load(q, w);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool ok = j < q.n;
            const uint32_t a = w[j] >> 24;
            if (level0) {
                wave_lo += (uint32_t)__popcll(__ballot(ok && a >= ref));
            } else if (SPIKES) {
                const bool zero = ok && a == 0, full = ok && a == 255;
                wave_lo += (uint32_t)__popcll(__ballot(zero));
                wave_hi += (uint32_t)__popcll(__ballot(full));
                if (ok && !zero && !full) atomicAdd(&bins[a], 1u);
            } else {
                if (ok) atomicAdd(&bins[a], 1u);
            }
        }
    }
    if ((threadIdx.x & 63) == 0) {
        if (wave_lo) atomicAdd(&bins[0], wave_lo);
        if (wave_hi) atomicAdd(&bins[255], wave_hi);
    }
    __syncthreads();
    const uint32_t v = bins[threadIdx.x];
    if (level0) {
        if (threadIdx.x == 0 && v) atomicAdd(&counts[img / levels], (unsigned long long)v);
    } else if (v) {
        atomicAdd(&hist[(int64_t)img * 256 + threadIdx.x], (unsigned long long)v);
    }
}

// one workgroup per (item, level >= 1); lane t owns threshold t
__global__ void __launch_bounds__(256)
mip_alpha_select_kernel(const AlphaImage* __restrict__ table, int32_t levels, uint32_t ref, const unsigned long long* __restrict__ counts,
                        const unsigned long long* __restrict__ hist, uint8_t* __restrict__ lut, itw_mip_coverage* __restrict__ report)
{
    __shared__ unsigned long long bins[256], ge[256], group[16], best;
    const int32_t item = (int32_t)(blockIdx.x / (uint32_t)(levels - 1)), level = 1 + (int32_t)(blockIdx.x % (uint32_t)(levels - 1));
    const int32_t img = item * levels + level;
    const uint32_t t = threadIdx.x;
    bins[t] = hist[(int64_t)img * 256 + t];
    if (t == 0) best = ~0ull;
    __syncthreads();
    unsigned long long above = 0;                                         // ge[t], the texels with a >= t: within t's group of 16 bins ...
    for (uint32_t u = t; u <= (t | 15u); u++) above += bins[u];
    if ((t & 15u) == 0) group[t >> 4] = above;
    __syncthreads();
    for (uint32_t g = (t >> 4) + 1; g < 16; g++) above += group[g];       // ... and the groups above it
    ge[t] = above;
    const unsigned long long n0 = (unsigned long long)table[item * levels].w * (unsigned long long)table[item * levels].h;
    const unsigned long long n = (unsigned long long)table[img].w * (unsigned long long)table[img].h;
    const unsigned long long cov0 = counts[item];
    const unsigned long long target = (cov0 * n + n0 / 2) / n0;       // (the entry point keeps cov0 * n within 64 bits)
    if (t >= 1) {
        const unsigned long long miss = above > target ? above - target : target - above;
        const uint32_t away = t > ref ? t - ref : ref - t;
        atomicMin(&best, (miss << 16) | ((unsigned long long)away << 8) | t);     // (|ge - K|, |t - r|, t), compared in that order
    }
    __syncthreads();
    const uint32_t chosen = (uint32_t)(best & 255u);
    lut[(int64_t)img * 256 + t] = (uint8_t)min(255u, t * ref / chosen);
    if (t == 0) {
        itw_mip_coverage row;
        row.texels = n; row.covered_plain = ge[ref]; row.covered = ge[chosen]; row.threshold = chosen; row.reserved = 0;
        report[img] = row;
        if (level == 1) {
            row.texels = n0; row.covered_plain = cov0; row.covered = cov0; row.threshold = ref;
            report[item * levels] = row;
        }
    }
}

__global__ void __launch_bounds__(256)
mip_alpha_rescale_kernel(const AlphaImage* __restrict__ table, int32_t count, uint32_t ref, const uint8_t* __restrict__ lut,
                         const itw_mip_coverage* __restrict__ report)
{
    __shared__ uint8_t map[256];
    const int32_t img = alpha_image_of<true>(table, count, blockIdx.x);
    if (report[img].threshold == ref) return;                             // a' == a: nothing to store (the workgroup's: every lane leaves)
    const AlphaImage im = table[img];
    map[threadIdx.x] = lut[(int64_t)img * 256 + threadIdx.x];
    __syncthreads();
    const int64_t quads = (int64_t)((im.w + 3) >> 2) * im.h;
    const int64_t base = (int64_t)(blockIdx.x - im.first_rescale) * kAlphaQuads + threadIdx.x;
#pragma unroll 4
    for (int k = 0; k < 4 * kAlphaPasses; k++) {
        const AlphaQuad q = alpha_quad(im, base + k * 256, quads);
        if (q.n == 0) continue;
        uint32_t w[4];
        alpha_quad_load(q, w);
#pragma unroll
        for (int j = 0; j < 4; j++) w[j] = (w[j] & 0x00ffffffu) | ((uint32_t)map[w[j] >> 24] << 24);
        if (q.vec) {
            *reinterpret_cast<uint4*>(q.p) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) if (j < q.n) reinterpret_cast<uint32_t*>(q.p)[j] = w[j];
        }
    }
}

namespace {

// which histogram kernel runs: one LDS atomic per texel, which measured 2-5 % faster per coverage call than the per-wave spike counts on
// cut-out and on noise alpha alike (DESIGN.md 3.11 has the rows); the hooks build can ask for the other
bool g_hist_spikes = false;

void launch_hist(const AlphaImage* table, int count, int levels, int ref, uint32_t blocks, unsigned long long* counts, unsigned long long* hist, hipStream_t st)
{
    if (g_hist_spikes) hipLaunchKernelGGL(mip_alpha_hist_kernel<true>, dim3(blocks), dim3(256), 0, st, table, count, levels, (uint32_t)ref, counts, hist);
    else               hipLaunchKernelGGL(mip_alpha_hist_kernel<false>, dim3(blocks), dim3(256), 0, st, table, count, levels, (uint32_t)ref, counts, hist);
    ITW_CHECK(hipGetLastError());
}

// the work buffer of one coverage pass: [table] [counts, a word per item] [histograms, 256 words per image] -- uploaded in one copy, the
// words as zeros -- then [report rows] [tables a -> a']
struct CoverageLayout {
    size_t counts, hist, upload, report, lut, bytes;
    CoverageLayout(int items, int levels)
    {
        const size_t count = (size_t)items * levels;
        counts = count * sizeof(AlphaImage);
        hist = counts + (size_t)items * 8;
        upload = hist + count * 256 * 8;
        report = up256(upload);
        lut = report + count * sizeof(itw_mip_coverage);
        bytes = up256(lut + count * 256);
    }
};

} // namespace

size_t coverage_work_bytes(int items, int levels) { return CoverageLayout(items, levels).bytes; }
size_t coverage_report_offset(int items, int levels) { return CoverageLayout(items, levels).report; }

void launch_coverage(const MipImage* images, int items, int levels, int w, int h, int ref, uint8_t* work, hipStream_t st)
{
    const CoverageLayout lay(items, levels);
    const int count = items * levels;
    static thread_local std::vector<uint8_t> host;                        // grow-only; alive while the copy below is in flight
    host.assign(lay.upload, 0);
    AlphaImage* t = reinterpret_cast<AlphaImage*>(host.data());
    uint64_t first = 0, first_rescale = 0;
    for (int i = 0; i < count; i++) {
        const int l = i % levels, lw = mip_dim(w, l), lh = mip_dim(h, l);
        t[i].ptr = images[i].ptr; t[i].stride = images[i].stride; t[i].w = lw; t[i].h = lh;
        t[i].first = (uint32_t)first; t[i].first_rescale = (uint32_t)first_rescale;
        first += alpha_blocks(lw, lh);
        if (l) first_rescale += alpha_blocks(lw, lh);
    }
    if (first > 0x7fffffffull) fail_msg("the coverage passes: %d items of %d x %d are more workgroups than one launch covers", items, w, h);
    ITW_CHECK(hipMemcpyAsync(work, host.data(), lay.upload, hipMemcpyHostToDevice, st));
    const AlphaImage* table = reinterpret_cast<const AlphaImage*>(work);
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(work + lay.counts);
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(work + lay.hist);
    itw_mip_coverage* report = reinterpret_cast<itw_mip_coverage*>(work + lay.report);
    launch_hist(table, count, levels, ref, (uint32_t)first, counts, hist, st);
    hipLaunchKernelGGL(mip_alpha_select_kernel, dim3((unsigned)(items * (levels - 1))), dim3(256), 0, st, table, levels, (uint32_t)ref, counts, hist, work + lay.lut, report);
    ITW_CHECK(hipGetLastError());
    hipLaunchKernelGGL(mip_alpha_rescale_kernel, dim3((uint32_t)first_rescale), dim3(256), 0, st, table, count, (uint32_t)ref, work + lay.lut, report);
    ITW_CHECK(hipGetLastError());
}

} // namespace itw

extern "C" int itwAlphaCoverage(const rgba_surface* images, int count, int alpha_ref, uint64_t* covered)
{
    itw::clear_failure();
    const bool ok = itw::guarded([&] {
        if (count < 0) itw::fail_msg("itwAlphaCoverage: %d images", count);
        if (alpha_ref < 0 || alpha_ref > 255) itw::fail_msg("itwAlphaCoverage: alpha_ref %d (0 .. 255)", alpha_ref);
        if (count == 0) return;
        if (!images || !covered) itw::fail_msg("itwAlphaCoverage: null %s pointer", images ? "covered" : "images");
        if (count > 0x7fffffff / 64) itw::fail_msg("itwAlphaCoverage: %d images", count);
        itw::check_images("itwAlphaCoverage", "image", images, count, 4, 4);
        uint64_t blocks = 0;
        for (int i = 0; i < count; i++) blocks += itw::alpha_blocks(images[i].width, images[i].height);
        if (blocks > 0x7fffffffull) itw::fail_msg("itwAlphaCoverage: %d images are more workgroups than one launch covers", count);
        const bool dev = itw::all_one_pointer_kind("itwAlphaCoverage", "image", images, count);

        // the thread's buffer: [table] [counts] [staged images (host pointers)]
        hipStream_t st = (hipStream_t)itwGetStream();
        const size_t counts_off = (size_t)count * sizeof(itw::AlphaImage);
        static thread_local std::vector<uint8_t> host;
        host.assign(counts_off + (size_t)count * 8, 0);
        itw::AlphaImage* t = reinterpret_cast<itw::AlphaImage*>(host.data());
        const itw::StagingPlan plan(images, count, 4, dev, host.size());
        uint8_t* base = static_cast<uint8_t*>(itw::decode_scratch(plan.bytes, st));
        uint32_t first = 0;
        for (int i = 0; i < count; i++) {
            t[i] = itw::AlphaImage{plan.ptr(i, base), plan.stride(i), images[i].width, images[i].height, first, 0};
            first += itw::alpha_blocks(images[i].width, images[i].height);
        }
        itw::upload_staged(plan, base, st);
        ITW_CHECK(hipMemcpyAsync(base, host.data(), host.size(), hipMemcpyHostToDevice, st));
        unsigned long long* counts = reinterpret_cast<unsigned long long*>(base + counts_off);
        itw::launch_hist(reinterpret_cast<const itw::AlphaImage*>(base), count, 1, alpha_ref, first, counts, counts, st);
        ITW_CHECK(hipMemcpyAsync(covered, counts, (size_t)count * 8, hipMemcpyDeviceToHost, st));
        ITW_CHECK(hipStreamSynchronize(st));
        itw::decode_scratch_done(st);
    });
    return ok ? 0 : -1;
}

#ifdef ITW_TEST_HOOKS
extern "C" void itwTestAlphaHistVariant(int spikes) { itw::g_hist_spikes = spikes != 0; }
#endif
