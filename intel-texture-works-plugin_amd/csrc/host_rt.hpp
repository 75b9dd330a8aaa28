// host_rt.hpp -- host-side runtime helpers shared by the translation units of libispc_texcomp.so (defined in abi.hip).
//
// Error model.  The reference ABI is `void` and cannot fail (ispc_texcomp.h:104-107), and there is deliberately no CPU
// implementation behind this library.  A HIP failure (no device, out of memory, bad pointer) therefore has two
// possible outcomes, chosen by the host (itwSetErrorMode / ITW_ON_ERROR):
//   abort  (default)  diagnostic on stderr, abort() -- loud, never a silently wrong texture;
//   return            the ABI call returns without touching further state, the message is kept per host thread
//                     (itwLastError) and the bool-returning dispatch entry points return false.  A plug-in host that
//                     must not lose the user's document probes itwAvailable() first and checks itwLastError() after.
// Inside the library a failure is a C++ exception (itw::Failure) that every extern "C" entry point catches.
//
// Besides the error model: the slice count of the plugin's save loop (slice_count: one rule for abi.hip and dispatch.hip), a worker's share
// of a slice pipeline (SlicedPart), and what refine.hip / decode_chain.hip need of the calling thread's context.  Format facts are not here:
// bcn_format.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include "../../include/ispc_texcomp.h"
#include "image_list_host.hpp"

namespace itw {

struct Failure { char msg[384]; };

[[noreturn]] void fail_hip(const char* what, hipError_t e, const char* file, int line);
[[noreturn]] void fail_msg(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void report_failure(const Failure& f) noexcept;      // records the message; aborts in abort mode
void clear_failure() noexcept;

// ITW_FORMAT_BC6H_SIGNED is a decode code: every entry point that encodes says so, before any device work, in place of "unknown format"
inline void refuse_signed_bc6h(const char* who, int format_code)
{
    if (format_code == 0x8E8E)
        fail_msg("%s: format 0x8E8E (BC6H, signed reading) is a decode code: there is no signed BC6H encoder (DXGI 96 encodes the reference's unsigned-coded blocks)", who);
}

#define ITW_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) ::itw::fail_hip(#expr, e_, __FILE__, __LINE__); } while (0)

// Runs `body`; a Failure ends in report_failure().  Returns true on success.
template <class F>
inline bool guarded(F&& body) noexcept
{
    try { body(); return true; }
    catch (const Failure& f) { report_failure(f); }
    catch (...) { Failure f; std::snprintf(f.msg, sizeof f.msg, "unexpected C++ exception inside libispc_texcomp"); report_failure(f); }
    return false;
}

// Slices the plugin's save loop cuts a width x height surface into (IntelPlugin.cpp:851-865): pixels / slice_pixels, by default 0x40000
// pixels per slice, at least one.  Above kMaxSlices the encode entry points fail and itwSliceWindowFor clamps.
constexpr int64_t kMaxSlices = 1 << 24;
inline int64_t slice_count(int64_t width, int64_t height, int64_t slice_pixels)
{
    const int64_t slices = width * height / (slice_pixels > 0 ? slice_pixels : 0x40000);
    return slices < 1 ? 1 : slices;
}

// One worker's share of a pipelined slice loop (abi.hip compress_sliced; dispatch.hip deals the windows of itwCompressImageSliced to the pool's
// GPUs): the worker runs windows part, part + parts, ... on ITS device and streams, calls `retired(first_slice, end_slice, ctx)` when a window's
// bytes are in the target instead of polling the caller's progress function (the submitting thread does that, in order), and stops issuing
// once `*stop` is set.
struct SlicedPart {
    int part = 0, parts = 1;
    void (*retired)(int first_slice, int end_slice, void* ctx) = nullptr;
    const std::atomic<bool>* stop = nullptr;
    void* ctx = nullptr;
};
// the share `part` of the slice loop over `source` (format, settings and slice size as itwCompressImageSlicedEx takes them); false: stopped or failed
bool sliced_part(const rgba_surface* source, uint8_t* target, int dxgi_format, const void* settings, int64_t slice_pixels, const SlicedPart& part);
// windows a call is cut into, and W (slices per window); 0 windows: the pipeline is off
int sliced_windows(int dxgi_format, const void* settings, int width, int height, int64_t slice_pixels, int* window_slices);

// the checks of itwCompressImageChain that need no device (counts, null pointers, sizes, strides, format), as a Failure; for the literal
// loop of a caller's own CompressionFunc, which takes no settings
void chain_check(const rgba_surface* images, int count, const uint8_t* target, int dxgi_format);
// the same checks with the caller's settings, as itwCompressImageChainEx makes them (null BC7 / BC6H / ETC1 settings, the ETC1 threshold); for
// itwCompressImageMipped, which must refuse before it builds the chain
void chain_check_with(const rgba_surface* images, int count, const uint8_t* target, int dxgi_format, const void* settings);

// What itwCompressImageRefined (refine.hip) needs of the calling thread's context.
// encode_resident: the device-pointer path of CompressBlocksBC7 / BC6H -- same routing, same workspace -- for a format code and settings
// pointer as itwCompressImageChainEx takes them; asynchronous on the thread's stream (itwSetStream).
void encode_resident(int dxgi_format, const void* settings, const uint8_t* d_src, int64_t stride, int width, int height, uint8_t* d_dst);
// refine_scratch: the thread's grow-only device scratch `which` (0: sized by the surface, 1: sized by the list), at least `bytes` bytes,
// 256-B aligned; growing frees the old buffer, which waits for the device.  refine_count_word: the thread's two pinned host words.
void* refine_scratch(int which, size_t bytes);
uint32_t* refine_count_word();

// What itwDecodeChain (decode_chain.hip) needs: the thread's grow-only device buffer for the descriptor table and the staging of host
// pointers, at least `bytes` bytes, 256-B aligned.  A call on another stream than the last one first waits for the event that
// decode_scratch_done(st) recorded behind that call's work (the BC7 workspace's rule); growing frees the old buffer, which waits for the device.
void* decode_scratch(size_t bytes, hipStream_t st);
void decode_scratch_done(hipStream_t st);
// What a one-call save (mipgen.hip) keeps its device-side chain in: a buffer of its own with the same rules, since the stages the call runs
// use the decode scratch while the chain lives.
void* chain_scratch(size_t bytes, hipStream_t st);
void chain_scratch_done(hipStream_t st);

// One predicate for "the kernels can dereference this pointer": device AND managed allocations (abi.hip and
// dispatch.hip and the decode entry used to disagree on managed memory).  Unregistered host memory -> false.
bool is_device_pointer(const void* p) noexcept;

// The HIP-side half of image_list_host.hpp.
// A reported fault of image `s` as the entry point `who`'s failure; the noun is the image's name in the message, printf style ("base %d",
// "item %d level %d"), `texel_bytes` and `align` what image_fault was asked for.
[[noreturn]] void fail_image(const char* who, ImageFaultKind kind, const rgba_surface& s, int texel_bytes, int align, const char* noun, ...)
    __attribute__((format(printf, 6, 7)));
inline void check_images(const char* who, const char* noun, const rgba_surface* images, int count, int texel_bytes, int align)
{
    if (const ImageFault f = image_list_fault(images, count, texel_bytes, align))
        fail_image(who, f.kind, images[f.index], texel_bytes, align, "%s %d", noun, f.index);
}
// true when every image of the list is device (or managed) memory, false when every one is host memory, a failure otherwise; `more`: a
// second list of `count` that must be of the same kind (itwQuantizeNormalMapChain's targets)
bool all_one_pointer_kind(const char* who, const char* noun, const rgba_surface* images, int count, const rgba_surface* more = nullptr);

// The copies of a plan's host images, width x height each and nothing more, to and from their places in the buffer at `base`; nothing for
// device images.  upload_staged / download_staged: every image of the plan, in order.
void upload_image(const StagingPlan& p, uint8_t* base, int i, hipStream_t st);
void download_image(const StagingPlan& p, uint8_t* base, int i, hipStream_t st);
void upload_staged(const StagingPlan& p, uint8_t* base, hipStream_t st);
void download_staged(const StagingPlan& p, uint8_t* base, hipStream_t st);

} // namespace itw
