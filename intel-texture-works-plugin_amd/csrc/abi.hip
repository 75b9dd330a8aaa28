// abi.hip -- the extern "C" boundary of libispc_texcomp.so.
//
// Exports exactly the BC symbols of the reference's L1 layer
//   CompressBlocksBC1/BC3/BC6H/BC7   (ispc_texcomp.cpp:417-435)
//   GetProfile_*                     (ispc_texcomp.cpp:20-410)
// plus the itw* extensions of include/itw_amd.h.  The reference forwards these
// calls to ISPC-generated x86 code; here the device boundary (H2D / launch /
// D2H) sits at the same line.  There is no CPU implementation behind this file:
// a HIP failure is reported on stderr and the process aborts, or -- if the host opted in with itwSetErrorMode -- the
// call returns and the message waits in itwLastError() (host_rt.hpp).
//
// The host layer, top to bottom: ThreadCtx (per-thread streams, staging buffers, the workspace; release() frees all of it) -- Job (a BcnKind
// of bcn_format.hpp plus the settings; every size and rule that follows from the format is read from that table, the geometry of a surface
// from its surface_geometry) -- claim_workspace / workspace_used (the one way the workspace changes streams) -- launch() (format -> kernel
// launcher, in a LaunchShape) -- host_route() + compress() (one call: resident, combined, windows, or staged runs) -- window_target_blocks /
// slice_window (the one window size) -- WindowPipeline + run_windows (the one pipeline: compress_sliced's windows and chain_groups' groups) --
// compress_single_run / compress_runs (the staged runs, cut by host_runs.hpp; several runs borrow the pipeline) -- the small-call combiner --
// presets -- the extern "C" entry points.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../include/itw_amd.h"
#include "../../include/itw_bc45.h"
#include "../../include/itw_dispatch.h"
#ifdef ITW_TEST_HOOKS
#include "../../include/itw_test_hooks.h"
#endif
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>
#include "bcn_format.hpp"
#include "host_rt.hpp"
#include "host_runs.hpp"
#include "kernels.hpp"
#include "x86_math.hpp"

namespace itw {

namespace {
std::atomic<int> g_error_mode{-1};                 // -1 = not decided yet (ITW_ON_ERROR), 0 abort, 1 return
thread_local char t_last_error[384] = {0};
thread_local bool t_has_error = false;

int error_mode() noexcept
{
    int m = g_error_mode.load(std::memory_order_relaxed);
    if (m < 0) {
        const char* e = std::getenv("ITW_ON_ERROR");
        m = (e && !std::strcmp(e, "return")) ? 1 : 0;
        g_error_mode.store(m, std::memory_order_relaxed);
    }
    return m;
}
}

void fail_hip(const char* what, hipError_t e, const char* file, int line)
{
    (void)hipGetLastError();                        // do not let the sticky error poison the next call
    Failure f;
    std::snprintf(f.msg, sizeof f.msg, "%s failed: %s (%d) at %s:%d", what, hipGetErrorString(e), (int)e, file, line);
    throw f;
}

void fail_msg(const char* fmt, ...)
{
    Failure f;
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(f.msg, sizeof f.msg, fmt, ap);
    va_end(ap);
    throw f;
}

void report_failure(const Failure& f) noexcept
{
    std::snprintf(t_last_error, sizeof t_last_error, "%s", f.msg);
    t_has_error = true;
    if (error_mode() == 0) {
        std::fprintf(stderr, "libispc_texcomp (itw-amd): %s -- no CPU fallback, aborting (itwSetErrorMode(ITW_ON_ERROR_RETURN) "
                             "makes this call return instead)\n", f.msg);
        std::abort();
    }
}

void clear_failure() noexcept { t_has_error = false; t_last_error[0] = 0; }

bool is_device_pointer(const void* p) noexcept
{
    if (!p) return false;
    hipPointerAttribute_t a;
    std::memset(&a, 0, sizeof(a));
    hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) { (void)hipGetLastError(); return false; }   // plain malloc'd memory on older runtimes
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

[[noreturn]] void fail_image(const char* who, ImageFaultKind kind, const rgba_surface& s, int texel_bytes, int align, const char* noun, ...)
{
    char what[64];
    va_list ap;
    va_start(ap, noun);
    std::vsnprintf(what, sizeof what, noun, ap);
    va_end(ap);
    switch (kind) {
    case IMAGE_NULL_TEXELS: fail_msg("%s: %s has a null texel pointer", who, what);
    case IMAGE_SIZE:        fail_msg("%s: %s is %d x %d", who, what, s.width, s.height);
    case IMAGE_STRIDE:      fail_msg("%s: %s: stride %d < %lld bytes per row", who, what, s.stride, (long long)s.width * texel_bytes);
    default:                fail_msg("%s: %s: texels are not %d-byte aligned", who, what, align);
    }
}

bool all_one_pointer_kind(const char* who, const char* noun, const rgba_surface* images, int count, const rgba_surface* more)
{
    const bool dev = is_device_pointer(images[0].ptr);
    for (int i = 0; i < count; i++)
        if ((i && is_device_pointer(images[i].ptr) != dev) || (more && is_device_pointer(more[i].ptr) != dev))
            fail_msg("%s: %s %d is %s memory, %s 0 %s: all images must be host or all device pointers", who, noun, i, dev ? "host" : "device", noun,
                     dev ? "device" : "host");
    return dev;
}

void upload_image(const StagingPlan& p, uint8_t* base, int i, hipStream_t st)
{
    if (p.dev) return;
    const rgba_surface& s = p.images[i];
    ITW_CHECK(hipMemcpy2DAsync(p.ptr(i, base), (size_t)p.stride(i), s.ptr, (size_t)s.stride, p.row_bytes(i), (size_t)s.height, hipMemcpyHostToDevice, st));
}

void download_image(const StagingPlan& p, uint8_t* base, int i, hipStream_t st)
{
    if (p.dev) return;
    const rgba_surface& s = p.images[i];
    ITW_CHECK(hipMemcpy2DAsync(s.ptr, (size_t)s.stride, p.ptr(i, base), (size_t)p.stride(i), p.row_bytes(i), (size_t)s.height, hipMemcpyDeviceToHost, st));
}

void upload_staged(const StagingPlan& p, uint8_t* base, hipStream_t st) { for (int i = 0; i < p.count; i++) upload_image(p, base, i, st); }
void download_staged(const StagingPlan& p, uint8_t* base, hipStream_t st) { for (int i = 0; i < p.count; i++) download_image(p, base, i, st); }

} // namespace itw

namespace {
using itw::is_device_pointer;

void* grow(void*& buf, size_t& cap, size_t need)
{
    if (need > cap) {
        if (buf) { void* old = buf; buf = nullptr; cap = 0; ITW_CHECK(hipFree(old)); }
        size_t want = need + need / 4 + 4096;
        void* fresh = nullptr;
        ITW_CHECK(hipMalloc(&fresh, want));
        buf = fresh; cap = want;
    }
    return buf;
}

// A grow-only device buffer that is ordered across streams by an event of its own.  Work already queued on another stream may still be
// using it, so a claim from another stream than the last makes that stream wait for the event done() recorded behind the previous use
// (never for the caller's old stream handle, which may have been destroyed since -- ADVICE r01); uses on one stream are ordered by the
// stream itself.  Growing frees the buffer first, and hipFree waits for the device.
struct OrderedBuffer {
    void* ptr = nullptr; size_t cap = 0;
    hipStream_t stream = nullptr; bool used = false;    // of the last claim (the caller's handle: not the library's to destroy)
    hipEvent_t event = nullptr;
    void* claim(size_t bytes, hipStream_t st)
    {
        if (!event) ITW_CHECK(hipEventCreateWithFlags(&event, hipEventDisableTiming));
        if (used && stream != st) ITW_CHECK(hipStreamWaitEvent(st, event, 0));
        grow(ptr, cap, bytes);
        stream = st; used = true;
        return ptr;
    }
    void done(hipStream_t st) { ITW_CHECK(hipEventRecord(event, st)); }      // the buffer is used up to here on `st`
    void release() noexcept
    {
        if (ptr) (void)hipFree(ptr);
        if (event) (void)hipEventDestroy(event);
        *this = OrderedBuffer{};
    }
};

// Per host thread: stream for device-resident calls and grow-only staging
// buffers for host-pointer calls.  The reference is called from up to 64 pool
// threads at once (win32Threads.cpp:211-249); thread_local state keeps those
// calls independent without a lock.
struct ThreadCtx {
    hipStream_t user_stream = nullptr;     // itwSetStream
    hipStream_t own_stream  = nullptr;     // staging path: kernels (and the copies of single-chunk calls)
    hipStream_t copy_stream = nullptr;     // staging path: copies of chunked calls, overlapped with own_stream
    hipEvent_t  ev_in[8] = {}, ev_done[8] = {};
    void*  d_in = nullptr;  size_t in_cap = 0;
    void*  d_out = nullptr; size_t out_cap = 0;
    OrderedBuffer ws;                               // BC7 inter-family workspace, the wide BC6H shape's
    itw::Bc7Aux aux = {nullptr, nullptr, nullptr, 0, nullptr, false, nullptr, false};   // second stream + fork / join / mid events: the parallel parts of small
                                                    // BC7 calls, the second band of large ones, the second kernel stream of the window pipeline
    itw::Bc7Verdict verdict = {nullptr, nullptr, false, nullptr};   // the pilot's estimate of a staged host-pointer call's first run, left for the host (kernels.hpp)
    bool staged_wide = false;                       // what the last staged BC7 call's estimate said (the shape of this call's first run, until its own is in)
    void*  d_refine[2] = {nullptr, nullptr}; size_t refine_cap[2] = {0, 0};   // itwCompressImageRefined (refine.hip): per-surface scratch, per-list scratch
    uint32_t* refine_count = nullptr;               // ... and the two pinned words its list count (and "target met") are read back through
    OrderedBuffer decode;                           // itwDecodeChain and the texel stages: descriptor table and, for host pointers, staging
    OrderedBuffer chain;                            // the device-side chain of a one-call save (mipgen.hip), alive while its stages use `decode`
    int    device = -1;
    char   info[256] = {0};
    // Every buffer, stream, event and pinned word of the context, freed and forgotten: the one place a new resource is added to.  Best effort
    // (the destructor runs it, and the runtime may already be gone at process exit): errors are ignored.  The caller's stream handles
    // (user_stream, the buffers' last streams) are not the library's to destroy.
    void release() noexcept
    {
        auto free_dev = [](void*& p, size_t& cap) { if (p) (void)hipFree(p); p = nullptr; cap = 0; };
        auto drop = [](hipStream_t& s) { if (s) (void)hipStreamDestroy(s); s = nullptr; };
        auto forget = [](hipEvent_t& e) { if (e) (void)hipEventDestroy(e); e = nullptr; };
        free_dev(d_in, in_cap); free_dev(d_out, out_cap);
        ws.release(); decode.release(); chain.release();
        for (int k = 0; k < 2; k++) free_dev(d_refine[k], refine_cap[k]);
        if (refine_count) (void)hipHostFree(refine_count);
        refine_count = nullptr;
        drop(own_stream); drop(copy_stream);
        for (auto& e : ev_in) forget(e);
        for (auto& e : ev_done) forget(e);
        drop(aux.stream); forget(aux.fork); forget(aux.join); forget(aux.mid);
        forget(verdict.event);
        if (verdict.host_counts) (void)hipHostFree((void*)verdict.host_counts);
        verdict.host_counts = nullptr; verdict.host_counts_dev = nullptr;
    }
    ~ThreadCtx() { release(); }
};
thread_local ThreadCtx tls_own;
// A combiner leader (below) works in its DEVICE's shared context instead of its own: whichever of the caller's 8 or 64 pool threads happens to
// lead a burst would otherwise bring its own staging buffers, workspace, streams and pinned words -- tens of milliseconds of hipMalloc the first
// time each thread leads, and 64 copies of the buffers (round 6: BC7 `basic`, one whole-surface CompressImageMT from 64 pool threads: 14.0 -> 4 ms).
thread_local ThreadCtx* tls_lent = nullptr;
#define tls (*(tls_lent ? tls_lent : &tls_own))

// Per-thread resources belong to the device they were created on: a host thread that switches devices (hipSetDevice)
// drops them and starts over.
void bind_thread_to_current_device()
{
    int dev = 0;
    ITW_CHECK(hipGetDevice(&dev));
    if (tls.device == dev) return;
    tls.release();
    tls.device = dev;
}

// staging path: streams and events of this thread, created on first use
void ensure_device_ctx()
{
    bind_thread_to_current_device();
    if (!tls.own_stream) ITW_CHECK(hipStreamCreateWithFlags(&tls.own_stream, hipStreamNonBlocking));
    if (!tls.copy_stream) ITW_CHECK(hipStreamCreateWithFlags(&tls.copy_stream, hipStreamNonBlocking));
    for (auto& e : tls.ev_in) if (!e) ITW_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& e : tls.ev_done) if (!e) ITW_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
}

// What to encode with: the format as the table knows it (bcn_format.hpp: every size and rule that follows from the format is read there) and
// what the table cannot know -- the settings.  ETC1: itwCompressBlocksETC1, slices and chains; no trampoline, no combiner, no refine, no multi-GPU.
struct Job {
    itw::BcnKind kind = itw::BCN_NONE;
    const bc7_enc_settings*  s7 = nullptr;
    const bc6h_enc_settings* s6 = nullptr;
    int etc_threshold = 0;      // ETC1 only: fastSkipTreshold, >= 1 (a copy: the caller's etc_enc_settings need not outlive job_of)
    uint32_t normal_ops = 0;    // BC5 only (itwCompressNormalMapBC5): ITW_NORMAL_* applied as the kernel loads its texels; such a job is never offered to the combiner
    float alpha_ref = 0.5f;     // BC1A, BC2 and BC3_DXTEX (which read the flags only) (slices and chains; no block-level call, so no combiner): the caller's itw_bc1a_settings, copied --
    uint32_t bc_flags = 0;      // NULL settings: TEX_THRESHOLD_DEFAULT, no flags
};

// The workspace (BC7's inter-family one, the wide BC6H shape's) is per host thread: claimed on `st`, and used up to workspace_used(st).
void* claim_workspace(size_t bytes, hipStream_t st)
{
    bind_thread_to_current_device();
    return tls.ws.claim(bytes, st);
}
void workspace_used(hipStream_t st) { tls.ws.done(st); }

// A staged run of a host-pointer call: its upload / download overlap the neighbouring runs' kernels.  A BC7 run that is not a band
// (compress_runs() below: round 4's shape, and what content that needs modes 1/3 everywhere still gets) takes the wide shape up to 2^20
// blocks -- scans and single-subset modes side by side on two streams fill the gaps between runs better than a chain of dependent
// launches on one stream (8.75 -> 7.89 ms for a 4096^2 `slow` call in round 2).  Device-resident calls keep the deep shape above
// 262144 blocks (a fifth of the HBM traffic and workspace).
// ITW_STAGED_WIDE_MAX: up to how many blocks a staged run of a host-pointer BC7 call takes the wide launch shape (tuning knob)
int64_t staged_wide_max_blocks()
{
    static const int64_t v = [] { const char* e = std::getenv("ITW_STAGED_WIDE_MAX"); return e ? (int64_t)std::atoll(e) : ((int64_t)1 << 20); }();
    return v < 1 ? 1 : v;
}

// ITW_STAGED_VERDICT_THR: percent of the first staged run's sampled blocks the pilot's estimate may list for the remaining runs to stay deep bands
int staged_verdict_percent()
{
    static const int v = [] { const char* e = std::getenv("ITW_STAGED_VERDICT_THR"); return e ? std::atoi(e) : 80; }();
    return v;
}

void ensure_bc7_aux()
{
    if (tls.aux.stream) return;
    bind_thread_to_current_device();
    ITW_CHECK(hipStreamCreateWithFlags(&tls.aux.stream, hipStreamNonBlocking));
    ITW_CHECK(hipEventCreateWithFlags(&tls.aux.fork, hipEventDisableTiming));
    ITW_CHECK(hipEventCreateWithFlags(&tls.aux.join, hipEventDisableTiming));
    ITW_CHECK(hipEventCreateWithFlags(&tls.aux.mid, hipEventDisableTiming));
    ITW_CHECK(hipEventCreateWithFlags(&tls.verdict.event, hipEventDisableTiming));
    // two pinned, device-visible words the pilot's estimate kernel writes for the host (no copy, no stream: ADVICE r05)
    void* h = nullptr;
    ITW_CHECK(hipHostMalloc(&h, 2 * sizeof(int32_t), hipHostMallocMapped));
    void* d = nullptr;
    ITW_CHECK(hipHostGetDevicePointer(&d, h, 0));
    tls.verdict.host_counts = static_cast<volatile int32_t*>(h);
    tls.verdict.host_counts_dev = static_cast<int32_t*>(d);
}

// How launch() runs a BC7 surface; every other format ignores it (BC6H claims its own workspace).  WHOLE and STAGED claim the workspace on
// `st` and record its event behind the kernels; a staged run -- one of a host-pointer call's, above -- takes the wide shape up to
// staged_wide_max_blocks().  A BAND runs in the deep shape on `st` alone (Bc7Aux::single), in the slice of the workspace at `ws_off`, which the
// caller has claimed and ordered: a run that compress_runs() overlaps with its neighbours on two streams, a window, a chain's group.
// VERDICT_BAND also leaves the pilot's estimate for the host (tls.verdict); a PROBE leaves the estimate alone and encodes nothing (the run
// itself took the wide shape).
struct LaunchShape {
    enum Kind { WHOLE, STAGED, BAND, VERDICT_BAND, PROBE } kind = WHOLE;
    size_t ws_off = 0;
};
#ifdef ITW_TEST_HOOKS
static_assert(ITW_ROUTE_SHAPE_WHOLE + LaunchShape::PROBE == ITW_ROUTE_SHAPE_PROBE && ITW_ROUTE_SHAPE_WHOLE + LaunchShape::BAND == ITW_ROUTE_SHAPE_BAND, "itw_test_hooks.h lists the shapes in Kind's order");
#endif

void launch(const Job& j, const uint8_t* d_src, int64_t stride, int w, int h, uint8_t* d_dst, hipStream_t st, LaunchShape shape = {})
{
    switch (j.kind) {
    case itw::BCN_NONE: break;                        // (job_of has refused it)
    case itw::BCN_BC6HS: break;                       // (a decode kind: format_kind never gives it to a Job)
    case itw::BCN_BC1:  itw::launch_bc1(d_src, stride, w, h, d_dst, st); break;
    case itw::BCN_BC3:  itw::launch_bc3(d_src, stride, w, h, d_dst, st); break;
    case itw::BCN_BC7:
        ensure_bc7_aux();
        ITW_ROUTE_SEEN(ITW_ROUTE_SHAPE_WHOLE + (int)shape.kind);                // (the route witness's shapes are in LaunchShape::Kind's order)
        tls.aux.wide_max_blocks = shape.kind == LaunchShape::WHOLE ? 0 : staged_wide_max_blocks();
        {
            // the per-call fields of the shared aux block go back to their defaults however this call ends (a failure is a C++ exception here,
            // and under ITW_ON_ERROR_RETURN the thread lives on)
            struct Reset { itw::Bc7Aux& a; ~Reset() { a.single = false; a.verdict = nullptr; a.probe = false; } } reset{tls.aux};
            tls.aux.single = shape.kind >= LaunchShape::BAND;
            void* ws = tls.ws.ptr;
            if (tls.aux.single) {
                tls.aux.verdict = shape.kind >= LaunchShape::VERDICT_BAND ? &tls.verdict : nullptr;
                tls.aux.probe = shape.kind == LaunchShape::PROBE;
                if (tls.aux.verdict) tls.verdict.valid = false;
            } else {
                ws = claim_workspace(itw::bc7_workspace_bytes(w, h, tls.aux.wide_max_blocks, j.s7), st);
            }
            itw::launch_bc7(d_src, stride, w, h, d_dst, *j.s7, reinterpret_cast<float*>(static_cast<uint8_t*>(ws) + shape.ws_off), st, &tls.aux);
            if (!tls.aux.single) workspace_used(st);
        }
        break;
    case itw::BCN_BC6H: {
        // the wide shape's workspace is the per-thread workspace too (most calls need none)
        const size_t need = itw::bc6h_workspace_bytes(w, h, *j.s6);
        void* ws = need ? claim_workspace(need, st) : nullptr;
        itw::launch_bc6h(d_src, stride, w, h, d_dst, *j.s6, st, ws);
        if (need) workspace_used(st);
        break;
    }
    case itw::BCN_BC4:  itw::launch_bc4(d_src, stride, w, h, d_dst, st); break;
    case itw::BCN_BC5:
        if (j.normal_ops) itw::launch_bc5_normal(d_src, stride, w, h, d_dst, j.normal_ops, st);
        else              itw::launch_bc5(d_src, stride, w, h, d_dst, st);
        break;
    case itw::BCN_BC4S: itw::launch_bc4s(d_src, stride, w, h, d_dst, st); break;
    case itw::BCN_BC5S: itw::launch_bc5s(d_src, stride, w, h, d_dst, st); break;
    case itw::BCN_ETC1:
        if ((int64_t)(w / 4) * (h / 4) > (int64_t)INT32_MAX) itw::fail_msg("ETC1: %d x %d is more blocks than one launch covers", w, h);
        itw::launch_etc1(d_src, stride, w, h, d_dst, j.etc_threshold, st);
        break;
    case itw::BCN_BC1A: itw::launch_bc1a(d_src, stride, w, h, d_dst, j.alpha_ref, j.bc_flags, st); break;
    case itw::BCN_BC2:  itw::launch_bc2(d_src, stride, w, h, d_dst, j.bc_flags, st); break;
    case itw::BCN_BC3DX: itw::launch_bc3_dxtex(d_src, stride, w, h, d_dst, j.bc_flags, st); break;
    }
    ITW_CHECK(hipGetLastError());
}

bool coalesce_small_call(const Job& j, const rgba_surface* src, uint8_t* dst, int64_t blocks);
bool heavy_job(const Job& j);
int64_t window_target_blocks(int kind, bool heavy);
static int64_t bc7_window_min_blocks() { static const int64_t v = [] { const char* e = std::getenv("ITW_BC7_WINDOW_MIN"); return e ? (int64_t)std::atoll(e) : (int64_t)262144; }(); return v; }   // BC7 host-pointer calls from this size take windows (2048^2 `basic` 1.28 -> 1.17 ms, 2896^2 2.46 -> 1.97, `slow` 4.24 -> 3.13)
bool compress_sliced(const Job& j, const rgba_surface* src, uint8_t* dst, int slices, ItwProgressFunc* progress, void* user, int fixed_window = 0,
                     const itw::SlicedPart* share = nullptr, bool leave_verdict = false);

// texel rows of a host surface into the tight staging image
void upload_rows(uint8_t* d_rows, size_t pitch, const uint8_t* hs, int64_t stride, size_t row_bytes, size_t nrows, hipStream_t copy)
{
    if (stride >= (int64_t)row_bytes) {                      // (also for tight rows: measured faster than one linear pageable copy)
        ITW_CHECK(hipMemcpy2DAsync(d_rows, pitch, hs, (size_t)stride, row_bytes, nrows, hipMemcpyHostToDevice, copy));
    } else {
        // bottom-up (negative stride) or overlapping rows: the reference just indexes ptr + y*stride with a
        // signed stride (kernel.ispc:105-151), which a pitched copy cannot express -- stage row by row
        for (size_t y = 0; y < nrows; y++)
            ITW_CHECK(hipMemcpyAsync(d_rows + y * pitch, hs + (int64_t)y * stride, row_bytes, hipMemcpyHostToDevice, copy));
    }
}

// The route of one call, decided once.  `resident`: both pointers are the device's -- launched on the caller's stream, asynchronous.
// `combinable`: both are host memory -- the call is first offered to the combiner (below), which joins small calls made concurrently by
// several host threads into one.  What the combiner does not take, and every mixed call: `windows` >= 2 windows of the window pipeline
// (compress_sliced with no callback; `leave_verdict`: the first one also counts the pilot's estimate), or, `windows` == 0, the staged runs.
struct HostRoute { bool resident = false, combinable = false; int windows = 0; bool leave_verdict = false; };
struct HostKnobs { const char *chunks, *runs, *windows_off; };       // ITW_HOST_CHUNKS, ITW_HOST_RUNS, ITW_HOST_WINDOWS_OFF as the environment has them (null: unset)

HostRoute host_route(const Job& j, const itw::SurfaceGeometry& geo, bool src_dev, bool dst_dev, bool staged_wide, const HostKnobs& env)
{
    HostRoute r;
    r.resident = src_dev && dst_dev;
    r.combinable = !src_dev && !dst_dev;
    // Round 6: a large BC6H call, and a large BC7 call of a profile without an order verdict (everything but `slow`), takes the WINDOW pipeline
    // of the slice loop (compress_sliced below) with no callback: windows of ~131 072 blocks alternate between two kernel streams with the
    // neighbours' copies on the third -- measured against the staged runs at 4096^2: BC6H `slow` 4.83 -> 4.3 ms, BC7 `alpha_basic` 3.31 -> 2.9,
    // `alpha_veryfast` 2.46 -> 2.0, `basic` 3.93 -> 3.6 (profiles/r06_host_pointer_path.txt, r06_sliced_timing.jsonl).  The tuning knobs of the runs keep the runs.
    if (!r.combinable || itw::keeps_partial_blocks(j.kind) || env.chunks || env.runs || env.windows_off) return r;
    const bool bc7 = j.kind == itw::BCN_BC7, bc6h = j.kind == itw::BCN_BC6H;
    const int64_t blocks = geo.blocks();
    // A profile WITH an order verdict (`slow`) takes the windows while the last estimate says the bounded order pays (each window runs it on one
    // stream: 5.6 against 6.05 ms for the staged runs on the bench surface) and the staged runs -- whose remaining runs go wide -- while it
    // says nearly every block needs modes 1/3 (photographs: 7.3 against 7.6 ms as windows).  Either way the call leaves a fresh estimate.
    const bool verdict_profile = bc7 && itw::bc7_has_order_verdict(*j.s7);
    const bool bc7w = bc7 && blocks >= bc7_window_min_blocks() && itw::bc7_staged_bands_ok() && (!verdict_profile || !staged_wide);
    const bool bc6w = bc6h && blocks >= 262144 && j.s6->slow_mode;    // (the other BC6H profiles are PCIe-bound: 2.98 vs 3.02 ms, fewer copies win)
    if (!bc7w && !bc6w) return r;
    const int64_t per_window = window_target_blocks(j.kind, heavy_job(j));
    int64_t windows = (blocks + per_window / 2) / per_window;
    if (windows > geo.by) windows = geo.by;
    if (windows >= 2) { r.windows = (int)windows; r.leave_verdict = bc7w && verdict_profile; }
    return r;
}

void compress_single_run(const Job& j, const rgba_surface* src, uint8_t* dst, const itw::SurfaceGeometry& geo, bool src_dev, bool dst_dev);
void compress_runs(const Job& j, const rgba_surface* src, uint8_t* dst, const itw::SurfaceGeometry& geo, bool dst_dev, const itw::HostRuns& runs);

void compress(const Job& j, const rgba_surface* src, uint8_t* dst, bool may_coalesce = true)
{
    if (may_coalesce) itw::clear_failure();
    if (!src) itw::fail_msg("null surface");
    const itw::SurfaceGeometry geo = itw::surface_geometry(j.kind, src->width, src->height);
    if (geo.empty()) return;                          // nothing to encode: the reference's loops do not run either
    if (!src->ptr || !dst) itw::fail_msg("null texel or destination pointer");
    const bool src_dev = is_device_pointer(src->ptr), dst_dev = is_device_pointer(dst);
    const HostKnobs env{std::getenv("ITW_HOST_CHUNKS"), std::getenv("ITW_HOST_RUNS"), std::getenv("ITW_HOST_WINDOWS_OFF")};
    const HostRoute route = host_route(j, geo, src_dev, dst_dev, tls.staged_wide, env);

    if (route.resident) { launch(j, src->ptr, src->stride, src->width, src->height, dst, tls.user_stream); return; }
    if (may_coalesce && route.combinable && coalesce_small_call(j, src, dst, geo.blocks())) return;
    if (route.windows) { (void)compress_sliced(j, src, dst, route.windows, nullptr, nullptr, 1, nullptr, route.leave_verdict); return; }
    const itw::HostRuns runs = itw::host_runs(j.kind, geo.bx, geo.by, !src_dev, env.chunks, env.runs);
    if (runs.n == 1) compress_single_run(j, src, dst, geo, src_dev, dst_dev);
    else             compress_runs(j, src, dst, geo, dst_dev, runs);
}

// ---- the plugin's slice loop as a pipeline (include/itw_dispatch.h: itwCompressImageSlicedEx) -----------------------------
// IntelPlugin.cpp:851-879 cuts a save into 0x40000-pixel slices and makes one synchronous CompressImageMT/ST call per slice, polling
// SetProgress between them.  Restated literally on a GPU every slice is upload -> a latency-bound launch chain over 1/64 of the
// chip-filling work -> download -> synchronise (BC7 `basic`: 1 274 Mpix/s against 4 175 for one call over the surface).  Here the same
// slices, progress calls and early out run as a PIPELINE: consecutive slices form a WINDOW (the unit of upload / launch / download: about 131 072 blocks, 262 144 for the PCIe-bound formats and the heavy BC7 settings),
// window k's kernels run on stream k % 2 with its
// upload and the previous window's download on the copy stream, and `progress(i, slices)` is called for every slice i of a window -- in
// order, each call only after the slices before it are in `target` -- once that window's bytes have arrived.  A false return stops the
// job: nothing further is issued or copied back, the one window in flight is drained, and every slice below i (and the rest of i's own
// window, at most W - 1 slices more) stays written, like the reference's early out.
std::atomic<int> g_slice_window{0};                // itwSetSliceWindow: 0 = by format and size, -1 = no pipeline (the literal loop)

int slice_window_setting()
{
    int W = g_slice_window.load(std::memory_order_relaxed);
    if (W == 0) {
        static const int env = [] {
            const char* off = std::getenv("ITW_SLICED_PIPELINE");
            if (off && off[0] == '0') return -1;
            const char* e = std::getenv("ITW_SLICE_WINDOW");
            return e ? std::atoi(e) : 0;
        }();
        W = env;
    }
    return W;
}

// The blocks a window aims at -- the unit of upload / launch / download of the slice loop, a chain's group budget, the windows of a large
// host-pointer call.  BC7 / BC6H: a window must fill the chip (131 072 blocks = one block per lane of 2 waves per SIMD; up to three windows are
// in flight); ETC1 goes with them; BC1 / BC3 / BC4 / BC5 are PCIe-bound: fewer, larger copies.
// `heavy`: BC7 settings that scan every two-subset shape (`slow`, `alpha_slow`: bc7_scans_every_shape) -- twice the work per block and dependent
// launch chains twice as long: windows twice as large (4096^2 `slow`, ms per sliced call with 8 / 16 / 32 slices per
// window: bench surface 5.91 / 5.57 / 5.86, photograph 8.18 / 7.62 / 7.73)
int64_t window_target_blocks(int kind, bool heavy)
{
    const bool compute = kind == itw::BCN_BC7 || kind == itw::BCN_BC6H || kind == itw::BCN_ETC1;
    return (compute && !heavy) ? 131072 : 262144;
}
bool heavy_job(const Job& j) { return j.kind == itw::BCN_BC7 && j.s7 && itw::bc7_scans_every_shape(*j.s7); }

// W, slices per window
int slice_window(int kind, int64_t slice_blocks, int slices, bool heavy)
{
    int W = slice_window_setting();
    if (W <= 0) {
        const int64_t target = window_target_blocks(kind, heavy);
        const int64_t per = slice_blocks < 1 ? 1 : slice_blocks;
        W = (int)((target + per / 2) / per);
        // No cap by slice count (the first version kept >= 8 windows per job): a window is 0.3-1 ms of work, so a job long enough to show a
        // progress bar has many; and windows SMALLER than the target run the deep launch shape on a fraction of the chip -- 2048^2 `basic` with 8
        // windows of 32 768 blocks 1.79 ms, with 2 of 131 072 1.13 (one call 1.16); 1024^2 with 4 windows 1.12 ms, as one 0.48 (literal loop 0.85).
    }
    if (W < 1) W = 1;
    if (W > slices) W = slices;
    return W;
}

struct SliceRows { int64_t y0, y1; };
// rows of slice i of `slices` (IntelPlugin.cpp:861-865); the formats that keep partial blocks end the last slice at `height`
SliceRows slice_rows(int i, int slices, int height, bool keep_partial)
{
    SliceRows r;
    r.y0 = ((int64_t)i * height / slices) & ~(int64_t)3;
    r.y1 = ((int64_t)(i + 1) * height / slices) & ~(int64_t)3;
    if (r.y1 > height) r.y1 = height;
    if (i == slices - 1 && keep_partial) r.y1 = height;
    return r;
}

// ---- the window pipeline: what the slice loop (compress_sliced) and a chain's gather groups (chain_groups) run on ------------------------
// Window k's kernels run on kernel stream k % 2 (the thread's own stream and the second stream of the BC7 aux block), its upload and the
// previous window's download on the copy stream; a BC7 window runs the deep shape in slice k % 2 of the per-thread workspace.  Uploads and
// kernels are ordered through a ring of 8 event pairs indexed by the caller's LOCAL window number k (at most depth + 1 <= 5 windows are
// between issue and retire).  The object waits for all three streams when it goes out of scope: however the call ends (a failure is a C++
// exception here), nothing of it is left in flight on the thread's streams and buffers, and the workspace's event lies behind it.
// The staged runs of one call (compress_runs) take the same streams, ring and drain, with a workspace layout and a stream per run of their own.
struct WindowPipeline {
    hipStream_t k0, k1, cs;
    size_t ws_off[2] = {0, 0};
    bool ws_claimed = false;

    // `bc7_slice_bytes` > 0: two workspace slices of that size (one per kernel stream).  Whatever produced a device surface (or still reads
    // the destination) on the caller's stream comes first: `wait_for_user`.
    WindowPipeline(bool wait_for_user, size_t bc7_slice_bytes)
    {
        ensure_device_ctx();
        ensure_bc7_aux();
        k0 = tls.own_stream; k1 = tls.aux.stream; cs = tls.copy_stream;
        if (wait_for_user && tls.user_stream != k0) ITW_CHECK(hipStreamSynchronize(tls.user_stream));
        if (bc7_slice_bytes) {
            const size_t b = (bc7_slice_bytes + 255) & ~(size_t)255;
            ws_off[1] = b;
            claim(2 * b);
        }
    }
    void claim(size_t bytes) { (void)claim_workspace(bytes, k0); ws_claimed = true; }   // the workspace in a layout of the caller's, ahead of fork()
    WindowPipeline(const WindowPipeline&) = delete;
    ~WindowPipeline()
    {
        (void)hipStreamSynchronize(k0); (void)hipStreamSynchronize(k1); (void)hipStreamSynchronize(cs);
        if (ws_claimed && tls.ws.event) (void)hipEventRecord(tls.ws.event, k0);
        (void)hipGetLastError();
    }
    // the second kernel stream starts behind whatever is on the first by now (the workspace's ordering, a chain's descriptor table)
    void fork() const
    {
        ITW_CHECK(hipEventRecord(tls.aux.fork, k0));
        ITW_CHECK(hipStreamWaitEvent(k1, tls.aux.fork, 0));
    }
    void join() const                   // ... and everything on it back into the first
    {
        ITW_CHECK(hipEventRecord(tls.aux.join, k1));
        ITW_CHECK(hipStreamWaitEvent(k0, tls.aux.join, 0));
    }
    hipStream_t stream(int k) const { return (k & 1) ? k1 : k0; }
    size_t workspace(int k) const { return ws_off[k & 1]; }
    // Window k's texels are queued on the copy stream: its kernels (on `ks`: the staged runs pick their own stream) wait for them.
    void after_upload(int k, hipStream_t ks) const { ITW_CHECK(hipStreamWaitEvent(ks, tls.ev_in[k & 7], 0)); }
    void uploaded(int k, hipStream_t ks) const { ITW_CHECK(hipEventRecord(tls.ev_in[k & 7], cs)); after_upload(k, ks); }
    void uploaded(int k) const { uploaded(k, stream(k)); }
    void encoded(int k, hipStream_t ks) const { ITW_CHECK(hipEventRecord(tls.ev_done[k & 7], ks)); }   // everything of window k is queued
    void encoded(int k) const { encoded(k, stream(k)); }
    void wait_encoded(int k) const { ITW_CHECK(hipEventSynchronize(tls.ev_done[k & 7])); }       // a window written where it belongs
    void queue_fetch(int k, void* dst, const void* staged, size_t len, hipMemcpyKind kind) const // a staged window's download behind its kernels
    {
        ITW_CHECK(hipStreamWaitEvent(cs, tls.ev_done[k & 7], 0));
        ITW_CHECK(hipMemcpyAsync(dst, staged, len, kind, cs));
    }
    void fetch(int k, void* dst, const void* staged, size_t len, hipMemcpyKind kind) const       // ... returns when it is in `dst`
    {
        queue_fetch(k, dst, staged, len, kind);
        ITW_CHECK(hipStreamSynchronize(cs));
    }
};

// The pilot's estimate of the last VERDICT_BAND or PROBE, once its event has fired (`wait`: now; otherwise only if it already has): the estimate
// kernel's last workgroup wrote the two counts into this thread's pinned words before it ended.  What the next staged BC7 call's first run
// and route go by (tls.staged_wide).  False while there is nothing to read.
bool read_verdict(bool wait)
{
    if (!tls.verdict.valid) return false;
    if (wait) ITW_CHECK(hipEventSynchronize(tls.verdict.event));
    else if (hipEventQuery(tls.verdict.event) != hipSuccess) { (void)hipGetLastError(); return false; }
    const int32_t listed = tls.verdict.host_counts[0], sampled = tls.verdict.host_counts[1];
    if (sampled > 0) tls.staged_wide = (int64_t)listed * 100 > (int64_t)staged_verdict_percent() * sampled;
    return true;
}

// The driver: `depth` windows AHEAD of the one being retired are issued.  With two, when window k-1's kernels end, window k is running on the
// other stream and window k+1 -- same stream as k-1, behind it in stream order -- already has its texels on the device.  (With one window of
// lookahead the upload of k+1 only started after k-1 had been retired, and for its 0.16 ms the chip ran window k alone.  4096^2, 64 slices, ms
// per call with a lookahead of 1 / 2 / 3: `basic` 3.81 / 3.58 / 3.59, `alpha_basic` 3.20 / 2.86 / 2.94, `slow` 6.50 / 5.96 / 5.96, BC6H `slow`
// 4.35 / 4.29 / 4.27, BC1 1.48 / 1.50 / 1.49.)  Per window: stopped()? -> issue the one `depth` ahead -> retire(k) -> report(k).  False when
// `stopped` or `report` ended the job: the windows behind that one are in flight, ~WindowPipeline waits for them, their bytes are not copied back.
// Where the two callers differ, on purpose:
//   lookahead     the slice loop's comes from ITW_SLICE_LOOKAHEAD (1 .. 4, default 2); a chain's is 2
//   one window    one slice window, and a chain's lone group, run the ordinary call shape (compress() / launch() pick it by size), not a pipeline
//   the verdict   only the slice loop's first window may leave the pilot's estimate (`leave_verdict`)
//   stopping      only a share of the slice loop (one pipeline per GPU, dispatch.hip) is stopped from outside
//   staged runs   compress_runs (below) takes the pipeline's streams, events and drain but not this driver: nobody is reported to between its
//                 runs, so the host never waits there -- every run and download is queued, then the call waits once
template <class Stopped, class Issue, class Retire, class Report>
bool run_windows(int n, int depth, Stopped&& stopped, Issue&& issue, Retire&& retire, Report&& report)
{
    for (int k = 0; k < depth && k < n; k++) issue(k);
    for (int k = 0; k < n; k++) {
        if (stopped()) return false;
        if (k + depth < n) issue(k + depth);
        retire(k);
        if (!report(k)) return false;
    }
    return true;
}

// ---- the staged runs of a host-pointer call (compress() above: what is neither resident, combined nor windows) -------------------------
// One run: BC1/3/4/5 and ETC1 of any size (PCIe-bound), every small BC7 / BC6H call, every call with a device source.  Upload, kernels and
// download follow each other on the thread's own stream; no second stream, no pinned words: the plug-in's 64 pool threads make such calls.
void compress_single_run(const Job& j, const rgba_surface* src, uint8_t* dst, const itw::SurfaceGeometry& geo, bool src_dev, bool dst_dev)
{
    ensure_device_ctx();
    hipStream_t st = tls.own_stream;
    // the producer of a device surface, or a reader of the device destination, may still be running on the caller's stream
    if ((src_dev || dst_dev) && tls.user_stream != st) ITW_CHECK(hipStreamSynchronize(tls.user_stream));
    uint8_t* in = src_dev ? nullptr : (uint8_t*)grow(tls.d_in, tls.in_cap, geo.pitch * geo.rows);
    uint8_t* d_dst = dst_dev ? dst : (uint8_t*)grow(tls.d_out, tls.out_cap, geo.out_bytes);
    const LaunchShape shape{(!src_dev && !dst_dev) ? LaunchShape::STAGED : LaunchShape::WHOLE};
    // the workspace ahead of the upload (growing it frees it, and hipFree waits for the device); launch() finds it claimed
    const size_t need = j.kind == itw::BCN_BC7  ? itw::bc7_workspace_bytes(src->width, geo.by * 4, shape.kind == LaunchShape::STAGED ? staged_wide_max_blocks() : 0, j.s7)
                      : j.kind == itw::BCN_BC6H ? itw::bc6h_workspace_bytes(src->width, geo.by * 4, *j.s6) : 0;
    if (need) (void)claim_workspace(need, st);
    // A failure below is a C++ exception (and under ITW_ON_ERROR_RETURN the thread lives on): whatever this call has queued by then is drained
    // and the workspace's event recorded, so the next call finds d_in / d_out / the workspace free of work in flight.
    struct Drain {
        bool done; hipStream_t st;
        ~Drain() {
            if (done) return;
            (void)hipStreamSynchronize(st);
            if (tls.aux.stream) (void)hipStreamSynchronize(tls.aux.stream);
            if (tls.ws.event && tls.ws.used) (void)hipEventRecord(tls.ws.event, st);
            (void)hipGetLastError();
        }
    } drain{false, st};
    if (!src_dev) upload_rows(in, geo.pitch, src->ptr, src->stride, geo.row_bytes, geo.rows, st);
    launch(j, src_dev ? src->ptr : in, src_dev ? (int64_t)src->stride : (int64_t)geo.pitch, src->width, (int)geo.rows, d_dst, st, shape);
    if (!dst_dev) ITW_CHECK(hipMemcpyAsync(dst, d_dst, geo.out_bytes, hipMemcpyDeviceToHost, st));
    ITW_CHECK(hipStreamSynchronize(st));
    drain.done = true;
}

// Several runs (itw::host_runs: large BC7 / BC6H calls from host memory, and what the knobs ask for), on a WindowPipeline's streams, events and
// drain: run c's upload and run c-1's download on the copy stream overlap run c's kernels.
// Round 5: the runs of a BC7 call are BANDS -- run c's kernels go to stream (c + 1) % 2 (the first, short run to the second stream),
// each run in the deep shape with its own slice of the workspace, so that one run's launch tails are filled by its neighbour's work as
// soon as that neighbour's texels have arrived (the device-resident path does the same with the two halves of a surface, bc7.hip).
// Content where nearly every block still needs modes 1/3 (photographs) gains nothing from the bounded order, and for it the WIDE shape,
// one run after the other, overlaps staged runs better (8.1 against 7.4 ms per 4096^2 call, profiles/history/r05/r05c_*).  Which it is comes
// from the pilot's estimate (bc7.hip bc7_pilot_estimate): counted behind the first run's {0,2} scan when that run is a band, by a
// probe on the second stream when it is wide.  The host never waits for it: the first run takes the shape the PREVIOUS call's
// estimate asked for (successive calls of a save -- mip levels, slices -- hold similar content), later runs this call's as soon as
// it is in (polled under the uploads), and it is read once more behind the call's last synchronisation for the next call.
// ITW_STAGED_BANDS=0: round 4's runs, one after the other in the wide shape.
void compress_runs(const Job& j, const rgba_surface* src, uint8_t* dst, const itw::SurfaceGeometry& geo, bool dst_dev, const itw::HostRuns& runs)
{
    const int w = src->width;
    const bool bc7 = j.kind == itw::BCN_BC7, bc6h = j.kind == itw::BCN_BC6H;
    const size_t pitch = geo.pitch, block_row = (size_t)geo.bx * geo.bpb;
    const bool bands = bc7 && itw::bc7_staged_bands_ok();
    const LaunchShape wide{dst_dev ? LaunchShape::WHOLE : LaunchShape::STAGED};
    const int64_t wide_max = dst_dev ? 0 : staged_wide_max_blocks();

    WindowPipeline pipe(dst_dev, 0);                         // (a run's source is host memory; a device destination may still be read on the caller's stream)
    hipStream_t st = pipe.k0;
    uint8_t* in = (uint8_t*)grow(tls.d_in, tls.in_cap, pitch * geo.rows);
    uint8_t* d_dst = dst_dev ? dst : (uint8_t*)grow(tls.d_out, tls.out_cap, geo.out_bytes);
    itw::BandWorkspace ws;
    if (bands) {
        ws = itw::band_workspace(runs, [&](int rows, bool as_wide) { return itw::bc7_workspace_bytes(w, rows, as_wide ? staged_wide_max_blocks() : 1, j.s7); });
        pipe.claim(ws.total);
        pipe.fork();                                         // the other streams start behind whatever ordered the workspace on the first
    } else if (bc7 || bc6h) {
        // sized once for the most demanding run: growing it frees it, and hipFree waits for the runs in flight
        const size_t need = itw::host_runs_workspace(runs, [&](int rows) { return bc7 ? itw::bc7_workspace_bytes(w, rows, wide_max, j.s7) : itw::bc6h_workspace_bytes(w, rows, *j.s6); });
        if (need) pipe.claim(need);
    }
    bool shape_wide = bands && tls.staged_wide && itw::bc7_has_order_verdict(*j.s7);   // the shape of the next run (profiles without a verdict: bands)
    bool verdict_pending = false;
    for (int c = 0; c < runs.n; c++) {
        const size_t y0 = (size_t)runs.cut[c] * 4;
        const size_t nrows = std::min(geo.rows - y0, (size_t)runs.rows(c));
        if (c > 0 && verdict_pending && read_verdict(false)) { verdict_pending = false; shape_wide = tls.staged_wide; }   // this call's estimate, if it is in
        const bool band = bands && !shape_wide;
        hipStream_t run_st = (band && ((c + 1) & 1)) ? pipe.k1 : st;
        upload_rows(in + y0 * pitch, pitch, src->ptr + (int64_t)y0 * src->stride, src->stride, geo.row_bytes, nrows, pipe.cs);
        pipe.uploaded(c, run_st);
        const uint8_t* run_src = in + y0 * pitch;
        uint8_t* run_dst = d_dst + (size_t)runs.cut[c] * block_row;
        launch(j, run_src, (int64_t)pitch, w, (int)nrows, run_dst, run_st, band ? LaunchShape{c == 0 ? LaunchShape::VERDICT_BAND : LaunchShape::BAND, ws.band_off[c]} : wide);
        if (bands && c == 0 && shape_wide) {
            // the first run went wide: the estimate comes from a probe on the second stream, behind that run's texels
            pipe.after_upload(0, pipe.k1);
            launch(j, run_src, (int64_t)pitch, w, (int)nrows, run_dst, pipe.k1, LaunchShape{LaunchShape::PROBE, ws.probe_off});
        }
        if (bands && c == 0) verdict_pending = tls.verdict.valid;
        if (dst_dev) continue;
        pipe.encoded(c, run_st);
        if (c > 0) {                                         // download the previous run while this one computes
            const size_t off = (size_t)runs.cut[c - 1] * block_row;
            pipe.queue_fetch(c - 1, dst + off, d_dst + off, (size_t)(runs.cut[c] - runs.cut[c - 1]) * block_row, hipMemcpyDeviceToHost);
        }
    }
    if (!dst_dev) {
        const size_t off = (size_t)runs.cut[runs.n - 1] * block_row;
        pipe.fetch(runs.n - 1, dst + off, d_dst + off, geo.out_bytes - off, hipMemcpyDeviceToHost);
    }
    if (bands) { pipe.join(); workspace_used(st); }          // everything back into the first stream; the workspace's event behind all of it
    ITW_CHECK(hipStreamSynchronize(st));
    if (verdict_pending) (void)read_verdict(true);           // for the next call, if it was not in before
}

// returns true when every slice was encoded, false when `progress` stopped the job
// `fixed_window` > 0 fixes W (compress() passes 1: its "slices" are the windows).
// `share`: this thread runs only the windows share->part, + share->parts, ... (one pipeline per GPU of the pool, dispatch.hip) and reports them
// through share->retired instead of polling `progress`.
// `leave_verdict` (BC7 profiles with an order verdict, whole-surface host-pointer calls): the first window also counts the pilot's estimate, and the
// call ends by reading it into tls.staged_wide -- what the NEXT such call's shape goes by (compress()).
bool compress_sliced(const Job& j, const rgba_surface* src, uint8_t* dst, int slices, ItwProgressFunc* progress, void* user, int fixed_window,
                     const itw::SlicedPart* share, bool leave_verdict)
{
    if (!src) itw::fail_msg("null surface");
    const int w = src->width, h = src->height;
    const itw::SurfaceGeometry geo = itw::surface_geometry(j.kind, w, h);
    const bool keep_partial = itw::keeps_partial_blocks(j.kind), bc7 = j.kind == itw::BCN_BC7;
    if (slices < 1) slices = 1;
    auto poll = [&](int first, int last) {               // progress(i) for i in [first, last], i < slices; false = stop
        for (int i = first; i <= last && i < slices; i++)
            if (i > 0 && progress && !progress(i, slices, user)) return false;
        return true;
    };
    if (geo.empty()) return share ? true : poll(1, slices - 1);   // nothing to encode: the reference's loop still polls
    if (!src->ptr || !dst) itw::fail_msg("null texel or destination pointer");
    const size_t block_row = (size_t)geo.bx * geo.bpb, pitch = geo.pitch;
    const bool src_dev = is_device_pointer(src->ptr), dst_dev = is_device_pointer(dst);

    const int W = fixed_window > 0 ? (fixed_window < slices ? fixed_window : slices) : slice_window(j.kind, geo.blocks() / slices, slices, heavy_job(j));
    const int nwin = (slices + W - 1) / W;
    const int part = share ? share->part : 0, parts = share ? (share->parts < 1 ? 1 : share->parts) : 1;
    const int nlocal = part < nwin ? (nwin - part + parts - 1) / parts : 0;       // this thread's windows: part, part + parts, ...
    if (nlocal == 0) return true;
    if (nwin == 1 && !share && fixed_window == 0) {
        // one window = the whole surface: the ordinary call (which picks its launch shape by size: the wide one for small surfaces), then the polls
        compress(j, src, dst, false);
        if (src_dev && dst_dev) ITW_CHECK(hipStreamSynchronize(tls.user_stream));
        return poll(1, slices - 1);
    }

    // BC7: one slice of the per-thread workspace per kernel stream, sized for the tallest window (deep shape: `single` in launch())
    int64_t tallest = 0;
    for (int k = 0; bc7 && k < nwin; k++) {
        const int s1 = (k + 1) * W < slices ? (k + 1) * W : slices;
        tallest = std::max(tallest, slice_rows(s1 - 1, slices, h, false).y1 - slice_rows(k * W, slices, h, false).y0);
    }
    WindowPipeline pipe(src_dev || dst_dev, bc7 ? itw::bc7_workspace_bytes(w, (int)tallest, 1, j.s7) : 0);
    uint8_t* in = src_dev ? nullptr : (uint8_t*)grow(tls.d_in, tls.in_cap, pitch * geo.rows);
    const uint8_t* d_src = src_dev ? src->ptr : in;
    const int64_t d_stride = src_dev ? (int64_t)src->stride : (int64_t)pitch;
    // A device `target` is written by the kernels themselves -- unless `progress` can stop the job: the windows in flight at that moment must
    // not reach `target` (itw_dispatch.h), so they are encoded into the staging buffer and copied over as they retire, like a host target's.
    const bool direct = dst_dev && !(progress && !share);
    uint8_t* d_dst = direct ? dst : (uint8_t*)grow(tls.d_out, tls.out_cap, geo.out_bytes);
    pipe.fork();

    struct Window { int s0, s1; int64_t y0, y1; int row0, nb; };
    auto window = [&](int i) {                            // this thread's i-th window: part + i * parts of the call's
        const int k = part + i * parts;
        Window v;
        v.s0 = k * W; v.s1 = (k + 1) * W < slices ? (k + 1) * W : slices;
        v.y0 = slice_rows(v.s0, slices, h, keep_partial).y0;
        v.y1 = slice_rows(v.s1 - 1, slices, h, keep_partial).y1;
        v.row0 = (int)(v.y0 / 4);
        v.nb = (int)((v.y1 - v.y0 + 3) / 4);
        return v;
    };
    auto issue = [&](int i) {
        const Window v = window(i);
        if (v.y1 <= v.y0) return;
        const size_t nrows = (size_t)(v.y1 - v.y0);
        if (!src_dev) {
            upload_rows(in + (size_t)v.y0 * pitch, pitch, src->ptr + v.y0 * (int64_t)src->stride, src->stride, geo.row_bytes, nrows, pipe.cs);
            pipe.uploaded(i);
        }
        launch(j, d_src + v.y0 * d_stride, d_stride, w, (int)nrows, d_dst + (size_t)v.row0 * block_row, pipe.stream(i),
               LaunchShape{(leave_verdict && i == 0) ? LaunchShape::VERDICT_BAND : LaunchShape::BAND, pipe.workspace(i)});
        pipe.encoded(i);
    };
    auto retire = [&](int i) {                            // the window's bytes into `dst`; returns when they are there
        const Window v = window(i);
        if (v.y1 <= v.y0) return;
        const size_t off = (size_t)v.row0 * block_row;
        if (direct) pipe.wait_encoded(i);
        else pipe.fetch(i, dst + off, d_dst + off, (size_t)v.nb * block_row, dst_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost);
    };
    auto report = [&](int i) {
        const Window v = window(i);
        if (!share) return poll(v.s0 + 1, v.s1);
        if (share->retired) share->retired(v.s0, v.s1, share->ctx);
        return true;
    };
    static const int depth = [] { const char* e = std::getenv("ITW_SLICE_LOOKAHEAD"); const int v = e ? std::atoi(e) : 2; return v < 1 ? 1 : (v > 4 ? 4 : v); }();
    auto stopped = [&] { return share && share->stop && share->stop->load(std::memory_order_acquire); };
    if (!run_windows(nlocal, depth, stopped, issue, retire, report)) return false;
    if (leave_verdict) (void)read_verdict(true);         // the first window's estimate, for the next call (its kernel is long done: every window has been retired)
    return true;
}

// format code + settings pointer of the dispatch layer -> Job (BC7 / BC6H: the settings struct must outlive the job; ETC1's threshold is copied)
Job job_of(int dxgi_format, const void* settings)
{
    Job j;
    itw::refuse_signed_bc6h("encode", dxgi_format);
    j.kind = itw::format_kind(dxgi_format);
    switch (j.kind) {
    case itw::BCN_NONE: itw::fail_msg("DXGI format %d is not one this library encodes", dxgi_format);
    case itw::BCN_BC7:  j.s7 = static_cast<const bc7_enc_settings*>(settings); break;
    case itw::BCN_BC6H: j.s6 = static_cast<const bc6h_enc_settings*>(settings); break;
    case itw::BCN_ETC1: {
        const etc_enc_settings* se = static_cast<const etc_enc_settings*>(settings);
        if (!se) itw::fail_msg("null settings for an ETC1 job");
        if (se->fastSkipTreshold < 1)
            itw::fail_msg("ETC1: fastSkipTreshold %d (1 .. 165; the reference emits uninitialised storage below 1)", se->fastSkipTreshold);
        j.etc_threshold = se->fastSkipTreshold;                               // (above 165: launch_etc1 takes 165)
        break;
    }
    case itw::BCN_BC1A:
    case itw::BCN_BC2:
    case itw::BCN_BC3DX: {                                                    // the same struct and checks; BC2 and BC3 have no colour key: alpha_ref is checked, not read
        const char* who = j.kind == itw::BCN_BC2 ? "BC2" : j.kind == itw::BCN_BC3DX ? "BC3 (DirectXTex)" : "BC1A";
        const itw_bc1a_settings* sb = static_cast<const itw_bc1a_settings*>(settings);
        if (!sb) break;                                                       // alpha_ref 0.5f, no flags
        if (sb->struct_size != sizeof(itw_bc1a_settings)) itw::fail_msg("%s: itw_bc1a_settings.struct_size %u (16)", who, sb->struct_size);
        if (sb->reserved != 0) itw::fail_msg("%s: itw_bc1a_settings.reserved %u (0)", who, sb->reserved);
        if (sb->flags & ~(uint32_t)(ITW_BC_DITHER_RGB | ITW_BC_DITHER_A | ITW_BC_UNIFORM)) itw::fail_msg("%s: unknown flag bits 0x%x", who, sb->flags);
        if (!std::isfinite(sb->alpha_ref)) itw::fail_msg("%s: alpha_ref is not finite", who);
        j.alpha_ref = sb->alpha_ref;
        j.bc_flags = sb->flags;
        break;
    }
    default: break;                                                           // BC1 / BC3 / BC4 / BC5 and the SNORM pair take no settings
    }
    if ((j.kind == itw::BCN_BC7 || j.kind == itw::BCN_BC6H) && !settings) itw::fail_msg("null settings for a BC7 / BC6H job");
    return j;
}

// the plugin's slice count; more than 2^24 slices is a bad call here (itwSliceWindowFor, which only reports, clamps instead)
int slices_of(const rgba_surface* s, int64_t slice_pixels)
{
    const int64_t slices = itw::slice_count(s->width, s->height, slice_pixels);
    if (slices > itw::kMaxSlices) itw::fail_msg("%lld slices", (long long)slices);
    return (int)slices;
}

// ---- a whole mip chain / cube map in one call (include/itw_dispatch.h: itwCompressImageChainEx) -----------------------------------
// IntelPlugin.cpp:229-255 pads and encodes every image of a ScratchImage -- each mip level of each face -- with its own call: upload, a
// latency-bound launch chain over a few thousand blocks, download, synchronise (66 of them for a 1024^2 cube map with mips).  Here the
// images are cut into GROUPS of consecutive images of up to a window's worth of blocks (window_target_blocks), each group is gathered
// into one packed surface (chain.hip) and encoded as one surface, and the groups are the windows of a WindowPipeline, as the slice loop's
// are.  An image of a window or more whose size is a multiple of 4 needs no gather: it is encoded in place through the whole-surface path
// (compress() / launch()).
constexpr int kChainPackedBlocks = 1024;              // P: blocks per packed row (the tail of the last row is encoded into scratch and dropped)

// everything a bad call can be told by before any device is touched (the pointer kinds come after this)
Job chain_job(const rgba_surface* images, int count, const uint8_t* target, int dxgi_format, const void* settings)
{
    if (count <= 0) itw::fail_msg("itwCompressImageChain: %d images", count);
    if (!images || !target) itw::fail_msg("itwCompressImageChain: null images or target pointer");
    const Job j = job_of(dxgi_format, settings);
    itw::check_images("itwCompressImageChain", "image", images, count, itw::texel_bytes(j.kind), 0);
    return j;
}

struct ChainUnit { int i0, i1; int64_t b0, nb; bool in_place; };   // images [i0, i1), blocks [b0, b0 + nb) of the chain

// The gather groups units[u0, u1) of a chain whose pointer kinds are known, pipelined; `poll(i0, i1)` reports images [i0, i1) as written.
template <class Poll>
bool chain_groups(const Job& j, const rgba_surface* im, uint8_t* target, const std::vector<ChainUnit>& units, size_t u0, size_t u1,
                  bool src_dev, bool dst_dev, Poll&& poll, uint32_t normal_ops = 0, int signed_source = 0)
{
    const int px = itw::texel_bytes(j.kind), bpb = itw::block_bytes(j.kind);
    const int spx = signed_source ? signed_source : px;      // bytes per SOURCE texel (a signed normal source: 4, 8 or 16 into packed RGBA8_SNORM)
    const bool fill45 = itw::keeps_partial_blocks(j.kind);
    const int ngroups = (int)(u1 - u0);
    // layout: d_in = [staged texels (host images)] [packed surfaces] [descriptors], d_out = [encoded packed surfaces]
    struct Group { int i0, i1; int64_t b0, nb; int pbx, pby; size_t packed_off, out_off; };
    std::vector<Group> gs((size_t)ngroups);
    const int first_image = units[u0].i0, nimg = units[u1 - 1].i1 - first_image;
    const itw::StagingPlan staged(im + first_image, nimg, spx, src_dev, 0);
    size_t in_bytes = staged.bytes, out_bytes = 0;
    int tallest = 0, widest = 0;
    for (int g = 0; g < ngroups; g++) {
        const ChainUnit& u = units[u0 + (size_t)g];
        Group& G = gs[(size_t)g];
        G.i0 = u.i0; G.i1 = u.i1; G.b0 = u.b0; G.nb = u.nb;
        G.pbx = (int)std::min<int64_t>(kChainPackedBlocks, u.nb);
        G.pby = (int)((u.nb + G.pbx - 1) / G.pbx);
        G.packed_off = in_bytes;
        in_bytes += itw::up256((size_t)G.pby * 4 * ((size_t)G.pbx * 4 * px));
        G.out_off = out_bytes;
        out_bytes += itw::up256((size_t)G.pby * G.pbx * bpb);
        if (G.pby > tallest || (G.pby == tallest && G.pbx > widest)) { tallest = G.pby; widest = G.pbx; }
    }
    const size_t desc_off = in_bytes;
    in_bytes += (size_t)nimg * sizeof(itw::ChainImage);
    std::vector<itw::ChainImage> desc((size_t)nimg);     // (declared ahead of the pipeline: it is still there while the pipeline drains)

    // one lone group runs the ordinary call (launch shape by size, the second stream for its own parallel parts); several alternate
    // between the two kernel streams, each BC7 group in its own slice of the workspace (deep shape)
    const bool lone = ngroups == 1;
    const bool bc7_slices = j.kind == itw::BCN_BC7 && !lone;
    WindowPipeline pipe(src_dev || dst_dev, bc7_slices ? itw::bc7_workspace_bytes(widest * 4, tallest * 4, 1, j.s7) : 0);
    uint8_t* d_in = (uint8_t*)grow(tls.d_in, tls.in_cap, in_bytes);
    uint8_t* d_out = (uint8_t*)grow(tls.d_out, tls.out_cap, out_bytes);

    // the descriptor table, one copy for every group, ahead of both kernel streams
    for (int g = 0; g < ngroups; g++) {
        const Group& G = gs[(size_t)g];
        int64_t first = 0;
        for (int i = G.i0; i < G.i1; i++) {
            desc[(size_t)(i - first_image)] = itw::ChainImage{staged.ptr(i - first_image, d_in), staged.stride(i - first_image), im[i].width, im[i].height, first};
            first += itw::image_blocks(im[i]);
        }
    }
    ITW_CHECK(hipMemcpyAsync(d_in + desc_off, desc.data(), desc.size() * sizeof(itw::ChainImage), hipMemcpyHostToDevice, pipe.k0));
    pipe.fork();

    const itw::ChainImage* d_desc = reinterpret_cast<const itw::ChainImage*>(d_in + desc_off);
    auto issue = [&](int g) {
        const Group& G = gs[(size_t)g];
        hipStream_t ks = pipe.stream(g);
        if (!src_dev) {
            for (int k = G.i0 - first_image; k < G.i1 - first_image; k++)
                upload_rows(staged.ptr(k, d_in), (size_t)staged.stride(k), staged.images[k].ptr, staged.images[k].stride, staged.row_bytes(k),
                            (size_t)staged.images[k].height, pipe.cs);
            pipe.uploaded(g);
        }
        const int64_t pitch = (int64_t)G.pbx * 4 * px;
        uint8_t* packed = d_in + G.packed_off;
        itw::launch_chain_gather(d_desc + (G.i0 - first_image), G.i1 - G.i0, G.nb, G.pbx, G.pby, px, fill45, packed, pitch, ks, nullptr, normal_ops, signed_source);
        launch(j, packed, pitch, G.pbx * 4, G.pby * 4, d_out + G.out_off, ks,
               lone ? LaunchShape{(!src_dev && !dst_dev) ? LaunchShape::STAGED : LaunchShape::WHOLE} : LaunchShape{LaunchShape::BAND, pipe.workspace(g)});
        if (dst_dev) ITW_CHECK(hipMemcpyAsync(target + G.b0 * bpb, d_out + G.out_off, (size_t)G.nb * bpb, hipMemcpyDeviceToDevice, ks));
        pipe.encoded(g);
    };
    auto retire = [&](int g) {                               // the group's bytes into `target`; returns when they are there
        const Group& G = gs[(size_t)g];
        if (dst_dev) pipe.wait_encoded(g);
        else pipe.fetch(g, target + G.b0 * bpb, d_out + G.out_off, (size_t)G.nb * bpb, hipMemcpyDeviceToHost);
    };
    return run_windows(ngroups, 2, [] { return false; }, issue, retire, [&](int g) { return poll(gs[(size_t)g].i0, gs[(size_t)g].i1); });
}

// `images` / `count` / `target` checked by chain_job.  Returns true when every image was encoded, false when `progress` stopped the job.
// `normal_ops` (itwCompressNormalMapChain): the gather prepares every texel it copies, so no image is encoded in place.
// `signed_source` (itwCompressSignedNormalMapChain): the images are signed normal sources of that many bytes per texel, quantised by the gather.
bool compress_chain(const Job& j, const rgba_surface* im, int count, uint8_t* target, ItwProgressFunc* progress, void* user, uint32_t normal_ops = 0,
                    int signed_source = 0)
{
    const bool src_dev = itw::all_one_pointer_kind("itwCompressImageChain", "image", im, count);
    if (src_dev) {
        int cur = 0, dev = 0;
        ITW_CHECK(hipGetDevice(&cur));
        for (int i = 0; i < count; i++) {
            hipPointerAttribute_t a;
            std::memset(&a, 0, sizeof a);
            ITW_CHECK(hipPointerGetAttributes(&a, im[i].ptr));
            dev = a.device;
            if (a.type == hipMemoryTypeDevice && dev != cur)
                itw::fail_msg("itwCompressImageChain: image %d lives on device %d, the calling thread's current device is %d", i, dev, cur);
        }
    }
    const bool dst_dev = is_device_pointer(target);
    const int bpb = itw::block_bytes(j.kind);

    // units, in order: in-place images, and groups of consecutive images of up to `budget` blocks
    const int64_t budget = window_target_blocks(j.kind, heavy_job(j));
    std::vector<ChainUnit> units;
    int64_t off = 0;
    bool open = false;
    for (int i = 0; i < count; i++) {
        const int64_t nb = itw::image_blocks(im[i]);
        if (nb >= budget) {
            const bool aligned = (im[i].width & 3) == 0 && (im[i].height & 3) == 0 && normal_ops == 0 && signed_source == 0;
            units.push_back(ChainUnit{i, i + 1, off, nb, aligned});            // in place, or (needs padding) a group of its own
            open = false;
        } else if (open && units.back().nb + nb <= budget) {
            units.back().i1 = i + 1; units.back().nb += nb;
        } else {
            units.push_back(ChainUnit{i, i + 1, off, nb, false});
            open = true;
        }
        off += nb;
    }

    bool stopped = false;
    auto poll = [&](int i0, int i1) {                        // progress(i) once images < i are in `target`
        for (int i = i0 + 1; i <= i1; i++)
            if (progress && !progress(i, count, user)) { stopped = true; return false; }
        return true;
    };
    size_t u = 0;
    while (u < units.size()) {
        const ChainUnit& U = units[u];
        if (U.in_place) {
            const rgba_surface& s = im[U.i0];
            uint8_t* dst = target + U.b0 * bpb;
            if (src_dev && dst_dev) {
                ITW_CHECK(hipStreamSynchronize(tls.user_stream));
                launch(j, s.ptr, s.stride, s.width, s.height, dst, tls.user_stream);
                ITW_CHECK(hipStreamSynchronize(tls.user_stream));
            } else {
                compress(j, &s, dst, false);               // host pointers: compress()'s windows (synchronous)
            }
            if (!poll(U.i0, U.i1)) return false;
            u++;
            continue;
        }
        size_t v = u;
        while (v < units.size() && !units[v].in_place) v++;
        if (!chain_groups(j, im, target, units, u, v, src_dev, dst_dev, poll, normal_ops, signed_source) || stopped) return false;
        u = v;
    }
    return true;
}

// ---- joining concurrent small calls ----------------------------------------------------------------------------------
// The reference's dispatch layer cuts every 0x40000-pixel slice into one band per pool thread and calls the ABI from all
// of them at once (win32Threads.cpp:211-249: 64 threads -> 64 calls of 8 texel rows at 4096 wide).  Each such call alone
// is a few workgroups plus two PCIe copies and a synchronisation -- 4096 of them per 4096^2 image.  Concurrent small
// host-pointer calls are therefore combined ("flat combining"): a caller queues its request; whoever finds no leader
// becomes the leader, takes everything queued for its device, merges requests that continue each other in memory (same
// format, settings, width and stride; src and dst of the next band start where the previous one ends -- exactly what
// win32Threads.cpp:223-230 produces), runs the merged surfaces as ordinary calls on its own stream and staging buffers,
// marks the requests done and hands leadership on.  A single-threaded caller always finds the queue empty and pays one
// uncontended mutex.  ITW_COALESCE=0 disables it.
struct Pending {
    Job job;
    bc7_enc_settings s7;
    bc6h_enc_settings s6;
    rgba_surface src;
    uint8_t* dst = nullptr;
    bool done = false, failed = false;
    char msg[384] = {0};
};

// ITW_COALESCE_DEBUG=1: per device, at process exit: bursts, batches (leader rounds), requests, merged calls, microseconds leaders waited
struct CombinerStats { std::atomic<long long> bursts{0}, batches{0}, requests{0}, calls{0}, wait_us{0}; };
CombinerStats g_cstats;
bool combiner_debug()
{
    static const bool on = [] {
        const char* e = std::getenv("ITW_COALESCE_DEBUG");
        const bool v = e && e[0] == '1';
        if (v) std::atexit([] {
            std::fprintf(stderr, "itw combiner: %lld bursts, %lld batches, %lld requests, %lld merged calls, leaders waited %lld us\n", g_cstats.bursts.load(),
                         g_cstats.batches.load(), g_cstats.requests.load(), g_cstats.calls.load(), g_cstats.wait_us.load());
        });
        return v;
    }();
#ifdef ITW_TEST_HOOKS
    if (!on) return true;              // the hooks build always counts (itwTestCombinerCounters); the report at exit stays the variable's
#endif
    return on;
}
#ifdef ITW_TEST_HOOKS
std::atomic<long long> g_hold_timeouts{0};            // itwTestCombinerHold: holds that ended by their timeout
#endif

struct Combiner {
    std::mutex m;
    std::condition_variable cv;
    std::vector<Pending*> queue;
    bool leader = false;
    ThreadCtx* ctx = nullptr;          // the device's shared context: used by whoever leads (one thread at a time), created by the first leader, never freed
    int burst = 0;                     // requests served since the queue was last idle
    int expected = 1;                  // size of the previous burst: the reference's pool submits the same number of bands
                                       // for every slice (win32Threads.cpp:217-231), so the next burst will be this large too
#ifdef ITW_TEST_HOOKS
    int hold_requests = 0, hold_timeout_ms = 0;       // itwTestCombinerHold (one-shot): the next leader waits for this many queued requests
#endif
};
constexpr int kMaxDevices = 64;
Combiner g_combiner[kMaxDevices];
// Calls up to this size are combined.  65 536 until round 6 ("larger calls fill the chip on their own") -- but eight pool threads handing over a 4096^2
// surface make eight concurrent calls of 131 072 blocks, each staging through its own thread's buffers and streams: BC7 `slow` 7.8 ms against 5.8 for one
// call, `basic` 4.06 against 3.72 (profiles/r06_reference_caller_timing.jsonl before the change).  Merged they are one call, which takes the windows.
constexpr int64_t kCoalesceMaxBlocks = 524288;       // (two pool threads halve a 4096^2 surface into calls of this size)

bool coalescing_enabled()
{
    static const bool on = [] { const char* e = std::getenv("ITW_COALESCE"); return !(e && e[0] == '0'); }();
    return on;
}

bool same_settings(const Pending& a, const Pending& b)
{
    if (a.job.kind != b.job.kind) return false;
    if (a.job.kind == itw::BCN_BC7) {
        // fields only: padding differs between stack objects, and refineIterations[7] is uninitialised storage in the RGB
        // presets (ispc_texcomp.cpp:20-189 never write it) -- it matters only when mode 7 runs (kernel.ispc:1419)
        const bc7_enc_settings &x = a.s7, &y = b.s7;
        for (int i = 0; i < 4; i++) if (x.mode_selection[i] != y.mode_selection[i]) return false;
        for (int i = 0; i < 7; i++) if (x.refineIterations[i] != y.refineIterations[i]) return false;
        const bool mode7 = x.mode_selection[1] && x.fastSkipTreshold_mode7 > 0;
        if (mode7 && x.refineIterations[7] != y.refineIterations[7]) return false;
        return x.skip_mode2 == y.skip_mode2 && x.fastSkipTreshold_mode1 == y.fastSkipTreshold_mode1 &&
               x.fastSkipTreshold_mode3 == y.fastSkipTreshold_mode3 && x.fastSkipTreshold_mode7 == y.fastSkipTreshold_mode7 &&
               x.mode45_channel0 == y.mode45_channel0 && x.refineIterations_channel == y.refineIterations_channel && x.channels == y.channels;
    }
    if (a.job.kind == itw::BCN_BC6H) {
        const bc6h_enc_settings &x = a.s6, &y = b.s6;
        return x.slow_mode == y.slow_mode && x.fast_mode == y.fast_mode && x.refineIterations_1p == y.refineIterations_1p &&
               x.refineIterations_2p == y.refineIterations_2p && x.fastSkipTreshold == y.fastSkipTreshold;
    }
    if (a.job.kind == itw::BCN_ETC1) return a.job.etc_threshold == b.job.etc_threshold;
    return true;
}

// b continues a: next rows of the same image, next block rows of the same stream
bool continues(const Pending& a, const Pending& b)
{
    if (!same_settings(a, b) || a.src.width != b.src.width || a.src.stride != b.src.stride) return false;
    if ((a.src.height & 3) || a.src.stride <= 0) return false;
    const itw::SurfaceGeometry geo = itw::surface_geometry(a.job.kind, a.src.width, a.src.height);
    return b.src.ptr == a.src.ptr + (int64_t)a.src.height * a.src.stride && b.dst == a.dst + (int64_t)(a.src.height / 4) * geo.bx * geo.bpb;
}

void run_batch(std::vector<Pending*>& batch)
{
    std::sort(batch.begin(), batch.end(), [](const Pending* a, const Pending* b) { return a->src.ptr < b->src.ptr; });
    // A chain's next request starts where its last one ends, so it lies further on in the sorted order -- as a rule right behind it, but the
    // bands of two surfaces that interleave in memory (the left and right halves of one image, two images sharing rows) alternate there:
    // the search goes on past requests that belong to another chain, up to the address the chain would continue at.
    std::vector<char> taken(batch.size(), 0);
    std::vector<Pending*> chain;
    for (size_t i = 0; i < batch.size(); i++) {
        if (taken[i]) continue;
        chain.assign(1, batch[i]);
        rgba_surface merged = batch[i]->src;
        for (size_t k = i + 1; k < batch.size() && merged.stride > 0; k++) {
            const Pending& last = *chain.back();
            if (batch[k]->src.ptr > last.src.ptr + (int64_t)last.src.height * last.src.stride) break;
            if (taken[k] || !continues(last, *batch[k]) || (int64_t)merged.height + batch[k]->src.height >= (1 << 30)) continue;
            taken[k] = 1;
            chain.push_back(batch[k]);
            merged.height += batch[k]->src.height;
        }
        Job j = batch[i]->job;
        j.s7 = &batch[i]->s7; j.s6 = &batch[i]->s6;
        if (combiner_debug()) g_cstats.calls++;
        try { compress(j, &merged, batch[i]->dst, false); }
        catch (const itw::Failure& f) {
            for (Pending* p : chain) { p->failed = true; std::snprintf(p->msg, sizeof p->msg, "%s", f.msg); }
        }
    }
}

bool coalesce_small_call(const Job& j, const rgba_surface* src, uint8_t* dst, int64_t blocks)
{
    if (blocks > kCoalesceMaxBlocks || !coalescing_enabled()) return false;
    bind_thread_to_current_device();
    if (tls.device < 0 || tls.device >= kMaxDevices) return false;
    Combiner& c = g_combiner[tls.device];
    Pending me;
    me.job = j;
    if (j.s7) me.s7 = *j.s7;
    if (j.s6) me.s6 = *j.s6;
    me.src = *src;
    me.dst = dst;

    std::unique_lock<std::mutex> lk(c.m);
    c.queue.push_back(&me);
    while (!me.done) {
        if (c.leader) { c.cv.wait(lk); continue; }
        c.leader = true;                                  // lead one batch (it contains this thread's request), then hand on
#ifdef ITW_TEST_HOOKS
        const bool held = c.hold_requests > 0;            // an armed hold takes the burst wait's place: the batch is what the test asked for
        if (held) {
            const int want = c.hold_requests;
            const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(c.hold_timeout_ms);
            c.hold_requests = 0;                          // one-shot
            while ((int)c.queue.size() < want) {
                if (std::chrono::steady_clock::now() >= deadline) { g_hold_timeouts++; break; }
                lk.unlock();
                const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(8);
                while (std::chrono::steady_clock::now() < until) std::this_thread::yield();
                lk.lock();
            }
        }
        if (!held)
#endif
        if (c.burst == 0 && c.expected > 1) {
            // start of a burst from a pool of threads released by one event: they arrive over some tens of microseconds.
            // Wait for as many requests as the previous burst had, as long as the queue keeps growing, so that the whole
            // slice becomes ONE merged call instead of a first small batch and a second one with the stragglers.
            const auto t0 = std::chrono::steady_clock::now();
            auto grown = t0;
            size_t seen = c.queue.size();
            while ((int)c.queue.size() < c.expected) {
                lk.unlock();
                const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(8);
                while (std::chrono::steady_clock::now() < until) std::this_thread::yield();
                lk.lock();
                const auto now = std::chrono::steady_clock::now();
                if (c.queue.size() != seen) { seen = c.queue.size(); grown = now; }
                if (now - grown > std::chrono::microseconds(80) || now - t0 > std::chrono::microseconds(600)) break;
            }
            if (combiner_debug()) g_cstats.wait_us += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
        }
        std::vector<Pending*> batch;
        batch.swap(c.queue);
        if (combiner_debug()) { g_cstats.batches++; g_cstats.requests += (long long)batch.size(); if (c.burst == 0) g_cstats.bursts++; }
        c.burst += (int)batch.size();
        lk.unlock();
        if (!c.ctx) c.ctx = new ThreadCtx;                // (only the leader touches c.ctx, and there is one leader at a time)
        tls_lent = c.ctx;
        try { run_batch(batch); }
        catch (...) {                                     // anything but an itw::Failure (those are caught per merged call):
            for (Pending* p : batch)                      // the requests must still be released and leadership handed on
                if (!p->failed) { p->failed = true; std::snprintf(p->msg, sizeof p->msg, "unexpected C++ exception while running a combined call"); }
        }
        tls_lent = nullptr;
        lk.lock();
        for (Pending* p : batch) p->done = true;
        if (c.queue.empty()) { c.expected = c.burst; c.burst = 0; }      // burst over
        c.leader = false;
        c.cv.notify_all();
    }
    lk.unlock();
    if (me.failed) { itw::Failure f; std::snprintf(f.msg, sizeof f.msg, "%s", me.msg); throw f; }
    return true;
}

// ---- quality presets (values: ispc_texcomp.cpp:20-410) ----------------------
struct Bc7Preset {
    int channels;
    bool sel[4];            // modes {0,2} {1,3,7} {4,5} {6}
    bool skip_mode2;
    int n1, n3, n7;         // partitions tried after PCA ranking
    int ch0, refine_channel;
    int refine[8];          // per mode; [7] < 0 = "left untouched" (the RGB profiles never write it)
};

constexpr Bc7Preset kUltrafast      {3, {false, false, false, true}, true,  3,  1,  0, 0, 0, {2, 2, 2, 1, 2, 2, 1, -1}};
constexpr Bc7Preset kVeryfast       {3, {false, true,  false, true}, true,  3,  1,  0, 0, 0, {2, 2, 2, 1, 2, 2, 1, -1}};
constexpr Bc7Preset kFast           {3, {false, true,  false, true}, true,  12, 4,  0, 0, 0, {2, 2, 2, 1, 2, 2, 2, -1}};
constexpr Bc7Preset kBasic          {3, {true,  true,  true,  true}, true,  12, 8,  0, 0, 2, {2, 2, 2, 2, 2, 2, 2, -1}};
constexpr Bc7Preset kSlow           {3, {true,  true,  true,  true}, false, 64, 64, 0, 0, 4, {4, 4, 4, 4, 4, 4, 4, -1}};
constexpr Bc7Preset kAlphaUltrafast {4, {false, false, true,  true}, true,  0,  0,  4, 3, 1, {2, 1, 2, 1, 1, 1, 2, 2}};
constexpr Bc7Preset kAlphaVeryfast  {4, {false, true,  true,  true}, true,  0,  0,  4, 3, 2, {2, 1, 2, 1, 2, 2, 2, 2}};
constexpr Bc7Preset kAlphaFast      {4, {false, true,  true,  true}, true,  4,  4,  8, 3, 2, {2, 1, 2, 1, 2, 2, 2, 2}};
constexpr Bc7Preset kAlphaBasic     {4, {true,  true,  true,  true}, true,  12, 8,  8, 0, 2, {2, 2, 2, 2, 2, 2, 2, 2}};
constexpr Bc7Preset kAlphaSlow      {4, {true,  true,  true,  true}, false, 64, 64, 64, 0, 4, {4, 4, 4, 4, 4, 4, 4, 4}};

void apply(const Bc7Preset& p, bc7_enc_settings* s)
{
    // field-wise on purpose: padding bytes and (for RGB presets) refineIterations[7]
    // keep whatever the caller had there, like the reference's assignment lists.
    s->channels = p.channels;
    for (int i = 0; i < 4; i++) s->mode_selection[i] = p.sel[i];
    s->skip_mode2 = p.skip_mode2;
    s->fastSkipTreshold_mode1 = p.n1;
    s->fastSkipTreshold_mode3 = p.n3;
    s->fastSkipTreshold_mode7 = p.n7;
    s->mode45_channel0 = p.ch0;
    s->refineIterations_channel = p.refine_channel;
    for (int i = 0; i < 8; i++) if (p.refine[i] >= 0) s->refineIterations[i] = p.refine[i];
}

struct Bc6hPreset { bool slow, fast; int n, r1p, r2p; };
void apply(const Bc6hPreset& p, bc6h_enc_settings* s)
{
    s->slow_mode = p.slow; s->fast_mode = p.fast;
    s->fastSkipTreshold = p.n; s->refineIterations_1p = p.r1p; s->refineIterations_2p = p.r2p;
}

// ---- device self-test kernels (libispc_texcomp_test.so only) ------------------
#ifdef ITW_TEST_HOOKS
__global__ void k_test_rcp(const float* in, float* out, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = itw::ispc_rcp(in[i], itw::global_seed_tables());
}
// Both implementations on every element: the general model on the global tables and the LDS fast path the BC7
// kernels use.  Where they disagree the output is corrupted on purpose so the oracle comparison fails.
__global__ void k_test_rsqrt(const float* in, float* out, int64_t n)
{
    __shared__ unsigned short s16[2048];
    __shared__ uint32_t s32[2048];
    const itw::SeedTables T = itw::stage_seed_tables_fast(s16, s32, threadIdx.x, blockDim.x);
    __syncthreads();
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float g = itw::ispc_rsqrt<false>(in[i], itw::global_seed_tables());
    const float f = itw::ispc_rsqrt<true>(in[i], T);
    const uint32_t gb = __float_as_uint(g), fb = __float_as_uint(f);
    out[i] = (gb == fb) ? g : ((g != g) ? 0.0f : __uint_as_float(gb ^ 1u));
}
__global__ void k_test_f2i(const float* in, int32_t* out, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = itw::f2i_x86(in[i]);
}
#endif // ITW_TEST_HOOKS

} // namespace

namespace itw {

bool sliced_part(const rgba_surface* source, uint8_t* target, int dxgi_format, const void* settings, int64_t slice_pixels, const SlicedPart& part)
{
    bool done = false;
    clear_failure();
    const bool ok = guarded([&] {
        if (!source) fail_msg("null surface");
        const Job j = job_of(dxgi_format, settings);
        done = compress_sliced(j, source, target, slices_of(source, slice_pixels), nullptr, nullptr, 0, &part);
    });
    return ok && done;
}

void chain_check(const rgba_surface* images, int count, const uint8_t* target, int dxgi_format)
{
    alignas(16) static const unsigned char any_settings[sizeof(bc7_enc_settings)] = {0};      // (the caller's own function takes none)
    static const etc_enc_settings any_etc = {1};
    const void* any = dxgi_format == ITW_FORMAT_ETC1_RGB8 ? (const void*)&any_etc : (format_kind(dxgi_format) == BCN_BC1A || format_kind(dxgi_format) == BCN_BC2 || format_kind(dxgi_format) == BCN_BC3DX) ? nullptr : (const void*)any_settings;
    (void)chain_job(images, count, target, dxgi_format, any);
}

void chain_check_with(const rgba_surface* images, int count, const uint8_t* target, int dxgi_format, const void* settings)
{
    (void)chain_job(images, count, target, dxgi_format, settings);
}

void encode_resident(int dxgi_format, const void* settings, const uint8_t* d_src, int64_t stride, int width, int height, uint8_t* d_dst)
{
    const Job j = job_of(dxgi_format, settings);
    launch(j, d_src, stride, width, height, d_dst, tls.user_stream);
}

void* refine_scratch(int which, size_t bytes)
{
    bind_thread_to_current_device();
    return grow(tls.d_refine[which], tls.refine_cap[which], bytes);
}

uint32_t* refine_count_word()
{
    bind_thread_to_current_device();
    if (!tls.refine_count) {
        void* h = nullptr;
        ITW_CHECK(hipHostMalloc(&h, 2 * sizeof(uint32_t), hipHostMallocDefault));    // the list length; itwCompressImageRefinedTo: and "target met"
        tls.refine_count = static_cast<uint32_t*>(h);
    }
    return tls.refine_count;
}

void* decode_scratch(size_t bytes, hipStream_t st)
{
    bind_thread_to_current_device();
    return tls.decode.claim(bytes, st);
}
void decode_scratch_done(hipStream_t st) { tls.decode.done(st); }

void* chain_scratch(size_t bytes, hipStream_t st)
{
    bind_thread_to_current_device();
    return tls.chain.claim(bytes, st);
}
void chain_scratch_done(hipStream_t st) { tls.chain.done(st); }

int sliced_windows(int dxgi_format, const void* settings, int width, int height, int64_t slice_pixels, int* window_slices)
{
    const int W = itwSliceWindowFor(dxgi_format, settings, width, height, slice_pixels);
    if (window_slices) *window_slices = W;
    if (W <= 0) return 0;
    return (int)((slice_count(width, height, slice_pixels) + W - 1) / W);
}

} // namespace itw

extern "C" {

void GetProfile_ultrafast(bc7_enc_settings* s) { apply(kUltrafast, s); }
void GetProfile_veryfast (bc7_enc_settings* s) { apply(kVeryfast, s); }
void GetProfile_fast     (bc7_enc_settings* s) { apply(kFast, s); }
void GetProfile_basic    (bc7_enc_settings* s) { apply(kBasic, s); }
void GetProfile_slow     (bc7_enc_settings* s) { apply(kSlow, s); }
void GetProfile_alpha_ultrafast(bc7_enc_settings* s) { apply(kAlphaUltrafast, s); }
void GetProfile_alpha_veryfast (bc7_enc_settings* s) { apply(kAlphaVeryfast, s); }
void GetProfile_alpha_fast     (bc7_enc_settings* s) { apply(kAlphaFast, s); }
void GetProfile_alpha_basic    (bc7_enc_settings* s) { apply(kAlphaBasic, s); }
void GetProfile_alpha_slow     (bc7_enc_settings* s) { apply(kAlphaSlow, s); }

void GetProfile_bc6h_veryfast(bc6h_enc_settings* s) { apply(Bc6hPreset{false, true,  0,  0, 0}, s); }
void GetProfile_bc6h_fast    (bc6h_enc_settings* s) { apply(Bc6hPreset{false, true,  2,  0, 1}, s); }
void GetProfile_bc6h_basic   (bc6h_enc_settings* s) { apply(Bc6hPreset{false, false, 4,  2, 2}, s); }
void GetProfile_bc6h_slow    (bc6h_enc_settings* s) { apply(Bc6hPreset{true,  false, 10, 2, 2}, s); }
void GetProfile_bc6h_veryslow(bc6h_enc_settings* s) { apply(Bc6hPreset{true,  false, 32, 2, 2}, s); }

void CompressBlocksBC1(const rgba_surface* src, uint8_t* dst)
{
    itw::guarded([&] { Job j; j.kind = itw::BCN_BC1; compress(j, src, dst); });
}
void CompressBlocksBC3(const rgba_surface* src, uint8_t* dst)
{
    itw::guarded([&] { Job j; j.kind = itw::BCN_BC3; compress(j, src, dst); });
}
void CompressBlocksBC7(const rgba_surface* src, uint8_t* dst, bc7_enc_settings* settings)
{
    itw::guarded([&] {
        if (!settings) itw::fail_msg("null bc7 settings");
        Job j; j.kind = itw::BCN_BC7; j.s7 = settings; compress(j, src, dst);
    });
}
void CompressBlocksBC6H(const rgba_surface* src, uint8_t* dst, bc6h_enc_settings* settings)
{
    itw::guarded([&] {
        if (!settings) itw::fail_msg("null bc6h settings");
        Job j; j.kind = itw::BCN_BC6H; j.s6 = settings; compress(j, src, dst);
    });
}

// ETC1 under the library's own prefix (include/itw_amd.h).  The call is never offered to the small-call combiner.
void itwGetProfile_etc_slow(etc_enc_settings* settings) { settings->fastSkipTreshold = 6; }      // ispc_texcomp.cpp:412-415
void itwCompressBlocksETC1(const rgba_surface* src, uint8_t* dst, const etc_enc_settings* settings)
{
    itw::clear_failure();
    itw::guarded([&] {
        if (!settings) itw::fail_msg("itwCompressBlocksETC1: null settings");
        if (settings->fastSkipTreshold < 1)
            itw::fail_msg("itwCompressBlocksETC1: fastSkipTreshold %d (1 .. 165; the reference emits uninitialised storage below 1)", settings->fastSkipTreshold);
        if (src && (int64_t)(src->width / 4) * (src->height / 4) > (int64_t)INT32_MAX)
            itw::fail_msg("itwCompressBlocksETC1: %d x %d is more blocks than one launch covers", src->width, src->height);
        Job j; j.kind = itw::BCN_ETC1; j.etc_threshold = settings->fastSkipTreshold;
        compress(j, src, dst, false);
    });
}

void CompressBlocksBC4(const rgba_surface* src, uint8_t* dst)
{
    itw::guarded([&] { Job j; j.kind = itw::BCN_BC4; compress(j, src, dst); });
}
void CompressBlocksBC5(const rgba_surface* src, uint8_t* dst)
{
    itw::guarded([&] { Job j; j.kind = itw::BCN_BC5; compress(j, src, dst); });
}
// BC5 of a normal map, the stages applied in the encoder's load (include/itw_bc45.h)
void itwCompressNormalMapBC5(const rgba_surface* src, uint8_t* dst, uint32_t ops)
{
    if (ops == 0) { CompressBlocksBC5(src, dst); return; }
    itw::clear_failure();
    itw::guarded([&] {
        itw::check_normal_ops("itwCompressNormalMapBC5", ops, "the fused load reads one block, and a texel's normal needs its neighbours");
        Job j; j.kind = itw::BCN_BC5; j.normal_ops = ops;
        compress(j, src, dst, false);
    });
}
void CompressBlocksBC4S(const rgba_surface* src, uint8_t* dst)
{
    itw::guarded([&] { Job j; j.kind = itw::BCN_BC4S; compress(j, src, dst); });
}
void CompressBlocksBC5S(const rgba_surface* src, uint8_t* dst)
{
    itw::guarded([&] { Job j; j.kind = itw::BCN_BC5S; compress(j, src, dst); });
}

// BC5_SNORM of a signed normal source, the definition applied in the encoder's load (include/itw_bc45.h).  A source of 8- or 16-byte texels
// does not fit the staging of the RGBA8 routes, so a host pointer is staged here: through the thread's buffer, on the caller's stream.
void itwCompressNormalMapBC5S(const rgba_surface* src, int texel_bytes, uint8_t* dst, uint32_t ops)
{
    if (texel_bytes == 4 && ops == 0) { CompressBlocksBC5S(src, dst); return; }
    itw::clear_failure();
    itw::guarded([&] {
        if (texel_bytes != 4 && texel_bytes != 8 && texel_bytes != 16) itw::fail_msg("itwCompressNormalMapBC5S: texel_bytes %d (4, 8 or 16)", texel_bytes);
        itw::check_normal_ops("itwCompressNormalMapBC5S", ops, "the fused load reads one block, and a texel's normal needs its neighbours");
        if (!src) itw::fail_msg("null surface");
        const int w = src->width, h = src->height;
        if (w <= 0 || h <= 0) return;                     // nothing to encode
        if (!src->ptr || !dst) itw::fail_msg("null texel or destination pointer");
        const int64_t bx = (w + 3) / 4, by = (h + 3) / 4;
        if (bx * by * 2 > (int64_t)INT32_MAX) itw::fail_msg("itwCompressNormalMapBC5S: %d x %d is more blocks than one launch covers", w, h);
        const bool src_dev = is_device_pointer(src->ptr), dst_dev = is_device_pointer(dst);
        if (src_dev && (((uintptr_t)src->ptr | (uintptr_t)(uint32_t)src->stride) & 3)) itw::fail_msg("itwCompressNormalMapBC5S: device texels not 4-byte aligned");
        hipStream_t st = tls.user_stream;
        if (src_dev && dst_dev) {                         // resident: one launch, asynchronous
            itw::launch_bc5s_normal(src->ptr, texel_bytes, src->stride, w, h, dst, ops, st);
            ITW_CHECK(hipGetLastError());
            return;
        }
        const size_t row_bytes = (size_t)w * (size_t)texel_bytes, pitch = (row_bytes + 15) & ~(size_t)15, out_bytes = (size_t)(bx * by) * 16;
        const size_t in_bytes = src_dev ? 0 : (pitch * (size_t)h + 255) & ~(size_t)255;
        uint8_t* base = static_cast<uint8_t*>(itw::decode_scratch(in_bytes + (dst_dev ? 0 : out_bytes), st));
        if (!src_dev) upload_rows(base, pitch, src->ptr, src->stride, row_bytes, (size_t)h, st);
        uint8_t* d_dst = dst_dev ? dst : base + in_bytes;
        itw::launch_bc5s_normal(src_dev ? src->ptr : base, texel_bytes, src_dev ? (int64_t)src->stride : (int64_t)pitch, w, h, d_dst, ops, st);
        ITW_CHECK(hipGetLastError());
        if (!dst_dev) ITW_CHECK(hipMemcpyAsync(dst, d_dst, out_bytes, hipMemcpyDeviceToHost, st));
        ITW_CHECK(hipStreamSynchronize(st));
        itw::decode_scratch_done(st);
    });
}

bool itwCompressImageSlicedEx(const rgba_surface* source, uint8_t* target, int64_t block_row_pitch, int dxgi_format, const void* settings,
                              int64_t slice_pixels, ItwProgressFunc* progress, void* user)
{
    bool done = false;
    itw::clear_failure();
    const bool ok = itw::guarded([&] {
        if (!source) itw::fail_msg("null surface");
        const Job j = job_of(dxgi_format, settings);
        const itw::SurfaceGeometry geo = itw::surface_geometry(j.kind, source->width, source->height);
        const int64_t tight = (int64_t)geo.bx * geo.bpb;
        if (block_row_pitch != tight) itw::fail_msg("itwCompressImageSlicedEx: block_row_pitch %lld != %lld (tight)", (long long)block_row_pitch, (long long)tight);
        done = compress_sliced(j, source, target, slices_of(source, slice_pixels), progress, user);
    });
    return ok && done;
}

bool itwCompressImageChainEx(const rgba_surface* images, int count, uint8_t* target, int dxgi_format, const void* settings,
                             ItwProgressFunc* progress, void* user)
{
    bool done = false;
    itw::clear_failure();
    const bool ok = itw::guarded([&] {
        const Job j = chain_job(images, count, target, dxgi_format, settings);
        done = compress_chain(j, images, count, target, progress, user);
    });
    return ok && done;
}

bool itwCompressNormalMapChain(const rgba_surface* images, int count, uint8_t* target, int dxgi_format, const void* settings, uint32_t ops,
                               ItwProgressFunc* progress, void* user)
{
    bool done = false;
    itw::clear_failure();
    const bool ok = itw::guarded([&] {
        itw::refuse_signed_bc6h("itwCompressNormalMapChain", dxgi_format);
        itw::check_normal_ops("itwCompressNormalMapChain", ops, "the gather works a texel at a time and has no neighbours");
        if (itw::format_kind(dxgi_format) == itw::BCN_BC1A) itw::fail_msg("itwCompressNormalMapChain: format 0x%X (BC1 with 1-bit alpha) holds colour, not normals", dxgi_format);
        if (itw::format_kind(dxgi_format) == itw::BCN_BC2) itw::fail_msg("itwCompressNormalMapChain: format 0x%X (BC2) holds colour, not normals", dxgi_format);
        if (itw::format_kind(dxgi_format) == itw::BCN_BC3DX) itw::fail_msg("itwCompressNormalMapChain: format 0x%X (BC3 by DirectXTex's encoder) holds colour, not normals", dxgi_format);
        const Job j = chain_job(images, count, target, dxgi_format, settings);
        done = compress_chain(j, images, count, target, progress, user, ops);
    });
    return ok && done;
}

// itwCompressImageChainEx for BC4_SNORM / BC5_SNORM over signed normal sources: the gather quantises every texel it copies (chain.hip)
bool itwCompressSignedNormalMapChain(const rgba_surface* images, int count, int texel_bytes, uint8_t* target, int dxgi_format, uint32_t ops,
                                     ItwProgressFunc* progress, void* user)
{
    bool done = false;
    itw::clear_failure();
    const bool ok = itw::guarded([&] {
        if (dxgi_format != 81 && dxgi_format != 84)
            itw::fail_msg("itwCompressSignedNormalMapChain: DXGI format %d (BC4_SNORM = 81 or BC5_SNORM = 84)", dxgi_format);
        if (texel_bytes != 4 && texel_bytes != 8 && texel_bytes != 16) itw::fail_msg("itwCompressSignedNormalMapChain: texel_bytes %d (4, 8 or 16)", texel_bytes);
        itw::check_normal_ops("itwCompressSignedNormalMapChain", ops, "the gather works a texel at a time and has no neighbours");
        const Job j = chain_job(images, count, target, dxgi_format, nullptr);
        itw::check_images("itwCompressSignedNormalMapChain", "image", images, count, texel_bytes, 0);
        done = compress_chain(j, images, count, target, progress, user, ops, texel_bytes);
    });
    return ok && done;
}

void itwSetSliceWindow(int slices) { g_slice_window.store(slices < 0 ? -1 : slices, std::memory_order_relaxed); }

int itwSliceWindow(int dxgi_format, int width, int height, int64_t slice_pixels) { return itwSliceWindowFor(dxgi_format, nullptr, width, height, slice_pixels); }

int itwSliceWindowFor(int dxgi_format, const void* settings, int width, int height, int64_t slice_pixels)
{
    if (slice_window_setting() < 0 || dxgi_format == ITW_FORMAT_BC6H_SIGNED) return 0;      // (a decode code: nothing encodes it, so no call has a window)
    const int kind = itw::format_kind(dxgi_format);         // (a code the library does not encode counts as PCIe-bound, dropping partial blocks)
    const int64_t slices = std::min(itw::slice_count(width, height, slice_pixels), itw::kMaxSlices);
    // null settings for BC7: not heavy
    const bool heavy = kind == itw::BCN_BC7 && settings && itw::bc7_scans_every_shape(*static_cast<const bc7_enc_settings*>(settings));
    return slice_window(kind, itw::surface_geometry(kind, width, height).blocks() / slices, (int)slices, heavy);
}

void  itwSetStream(void* s) { tls.user_stream = (hipStream_t)s; }
void* itwGetStream(void)    { return (void*)tls.user_stream; }

int itwAvailable(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) { (void)hipGetLastError(); return 0; }
    int dev = 0;
    hipDeviceProp_t p;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return std::strncmp(p.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;     // the only code object this library carries
}

void itwSetErrorMode(int mode) { itw::g_error_mode.store(mode == ITW_ON_ERROR_RETURN ? 1 : 0); }
const char* itwLastError(void) { return itw::t_has_error ? itw::t_last_error : nullptr; }
void itwClearError(void) { itw::clear_failure(); }

const char* itwDeviceInfo(void)
{
    tls.info[0] = 0;
    itw::guarded([&] {
        int dev = 0;
        ITW_CHECK(hipGetDevice(&dev));
        hipDeviceProp_t p;
        ITW_CHECK(hipGetDeviceProperties(&p, dev));
        std::snprintf(tls.info, sizeof(tls.info), "%s / %s / %d CUs / %.0f MHz", p.gcnArchName, p.name,
                      p.multiProcessorCount, p.clockRate / 1000.0);
    });
    return tls.info;
}

void itwSetBc7Path(int path) { itw::set_bc7_path(path); itw::set_bc6h_path(path); }
void itwSetBc7Pilot(int percent) { itw::set_bc7_pilot(percent); }

const char* itwVersion(void) { return "itw-amd 0.1 gfx950 arith=x86-lut-nr contract=off"; }

int64_t itwBandForPart(int32_t width, int32_t height, int32_t bytes_per_block,
                       int32_t part, int32_t parts, int32_t* first_row, int32_t* row_count)
{
    const int64_t R = height / 4, bx = width / 4;
    if (parts <= 0 || part < 0 || part >= parts) { if (first_row) *first_row = 0; if (row_count) *row_count = 0; return -1; }
    const int64_t r0 = R * part / parts, r1 = R * (part + 1) / parts;
    if (first_row) *first_row = (int32_t)(r0 * 4);
    if (row_count) *row_count = (int32_t)((r1 - r0) * 4);
    return r0 * bx * bytes_per_block;
}

int64_t itwBandForPartEx(int32_t width, int32_t height, int32_t bytes_per_block, int32_t part, int32_t parts, int32_t keep_partial_blocks,
                         int32_t* first_row, int32_t* row_count)
{
    if (!keep_partial_blocks) return itwBandForPart(width, height, bytes_per_block, part, parts, first_row, row_count);
    const int64_t R = ((int64_t)height + 3) / 4, bx = ((int64_t)width + 3) / 4;
    if (parts <= 0 || part < 0 || part >= parts || height < 1 || width < 1) { if (first_row) *first_row = 0; if (row_count) *row_count = 0; return -1; }
    const int64_t r0 = R * part / parts, r1 = R * (part + 1) / parts;
    const int64_t y0 = r0 * 4, y1 = (r1 * 4 < height) ? r1 * 4 : height;       // the band that holds the last block row keeps its partial rows
    if (first_row) *first_row = (int32_t)y0;
    if (row_count) *row_count = (int32_t)(y1 > y0 ? y1 - y0 : 0);
    return r0 * bx * bytes_per_block;
}

void itwWarmupBC45(void)
{
    itwClearError();
    itw::guarded([&] { bind_thread_to_current_device(); itw::warmup_bc45(); });
}

void itwWarmupBC45S(void)
{
    itwClearError();
    itw::guarded([&] { bind_thread_to_current_device(); itw::warmup_bc45s(); });
}

#ifdef ITW_TEST_HOOKS      // libispc_texcomp_test.so only (include/itw_test_hooks.h)
int itwTestBc45IndexTable(uint32_t* host_out)
{
    itwClearError();
    return itw::guarded([&] { if (!host_out) itw::fail_msg("null pointer"); itw::copy_bc45_index_table(host_out, tls.user_stream); }) ? 0 : -1;
}

int itwTestBc45ClosestS(uint8_t* host_out)
{
    itwClearError();
    return itw::guarded([&] { if (!host_out) itw::fail_msg("null pointer"); itw::copy_bc45_closest_snorm(host_out, tls.user_stream); }) ? 0 : -1;
}

int itwTestWalks32(int kind, int64_t stride, int width, int height)
{
    if (kind == 1 || kind == 3) return itw::bc13_walks_32(kind == 3, stride, width, height) ? 1 : 0;
    if (kind == 4 || kind == 8 || kind == 16) return itw::bc45_walks_32(kind, stride, width, height) ? 1 : 0;
    return -1;
}

void itwTestBc7TwoSubsetBounds(const rgba_surface* d_src, float* d_out)
{
    itwClearError();
    itw::guarded([&] {
        if (!d_src || !d_src->ptr || !d_out) itw::fail_msg("null pointer");
        itw::launch_bc7_test_bounds(d_src->ptr, d_src->stride, d_src->width, d_src->height, d_out, tls.user_stream);
        ITW_CHECK(hipGetLastError());
    });
}

void itwTestBc7RotationBounds(const rgba_surface* d_src, float* d_out)
{
    itwClearError();
    itw::guarded([&] {
        if (!d_src || !d_src->ptr || !d_out) itw::fail_msg("null pointer");
        itw::launch_bc7_test_rot_bounds(d_src->ptr, d_src->stride, d_src->width, d_src->height, d_out, tls.user_stream);
        ITW_CHECK(hipGetLastError());
    });
}

void itwTestBc7F02Scan(const rgba_surface* d_src, int32_t* d_out)
{
    itwClearError();
    itw::guarded([&] {
        if (!d_src || !d_src->ptr || !d_out) itw::fail_msg("null pointer");
        itw::launch_bc7_test_f02_scan(d_src->ptr, d_src->stride, d_src->width, d_src->height, d_out, tls.user_stream);
        ITW_CHECK(hipGetLastError());
    });
}

void itwTestRcp(const float* in, float* out, int64_t n)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_test_rcp, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, tls.user_stream, in, out, n);
    itw::guarded([&] { ITW_CHECK(hipGetLastError()); });
}
void itwTestRsqrt(const float* in, float* out, int64_t n)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_test_rsqrt, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, tls.user_stream, in, out, n);
    itw::guarded([&] { ITW_CHECK(hipGetLastError()); });
}
void itwTestF2I(const float* in, int32_t* out, int64_t n)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_test_f2i, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, tls.user_stream, in, out, n);
    itw::guarded([&] { ITW_CHECK(hipGetLastError()); });
}

void itwTestCombinerHold(int requests, int timeout_ms)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return; }
    if (dev < 0 || dev >= kMaxDevices) return;
    Combiner& c = g_combiner[dev];
    std::lock_guard<std::mutex> lk(c.m);
    c.hold_requests = requests > 0 ? requests : 0;
    c.hold_timeout_ms = timeout_ms > 0 ? timeout_ms : 0;
}

void itwTestCombinerCounters(int64_t out[5])
{
    if (!out) return;
    out[0] = g_cstats.bursts.load(); out[1] = g_cstats.batches.load(); out[2] = g_cstats.requests.load(); out[3] = g_cstats.calls.load();
    out[4] = g_hold_timeouts.load();
}

void itwTestBc7RouteCounters(int64_t* out, int n)
{
    if (out && n > 0) itw::bc7_route_counters(out, n);
}

void itwTestBc7RouteCountersReset(void) { itw::bc7_route_counters_reset(); }

void itwTestBc7CallCountersArm(int on) { itw::bc7_arm_call_counters(on); }
void itwTestBc7CallCounters(int32_t* out, int n)
{
    if (out && n > 0) itw::bc7_call_counters(out, n);
}
#endif // ITW_TEST_HOOKS

} // extern "C"
