/*
 * itw_test_hooks.h -- entry points of libispc_texcomp_test.so ONLY (csrc/Makefile target `test`: the same sources compiled with
 * -DITW_TEST_HOOKS).  The product library, libispc_texcomp.so, does not export them (tests/test_abi_boundary.py checks `nm -D`): a drop-in
 * DLL carries no test code (VERDICT r04 / ADVICE r04).  tests/ load the test build for exactly these calls and the product for everything
 * else.  Replaces nothing in the reference.
 */
#ifndef ITW_TEST_HOOKS_H
#define ITW_TEST_HOOKS_H

#include "ispc_texcomp.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)   /* the library is built with -fvisibility=hidden: only what the headers declare is exported */

/* The pinned arithmetic on the GPU (csrc/x86_math.hpp): rcp / rsqrt / float->int of `n` floats resident in HBM. */
void itwTestRcp  (const float* d_in, float* d_out, int64_t n);
void itwTestRsqrt(const float* d_in, float* d_out, int64_t n);
void itwTestF2I  (const float* d_in, int32_t* d_out, int64_t n);

/* The bounded BC7 mode order's lower bound (csrc/bc7_exact.hpp two_subset_bound): for every 4x4 block of the device-resident RGBA8
 * surface, the bound of each of the 64 two-subset shapes, d_out[block * 64 + shape] (device memory, raster block order).  tests/ check it
 * against the oracle's error of every shape (it must never exceed one) and against its CPU restatement (oracle/bc7_bound.c). */
void itwTestBc7TwoSubsetBounds(const rgba_surface* d_src, float* d_out);

/* The bound that lists modes 4/5's (block, rotation) pairs under an RGB profile (csrc/bc7_exact.hpp rotation_bound): for every 4x4 block
 * of the device-resident RGBA8 surface, the bound of rotations 0..2, d_out[block * 3 + rotation] (device memory, raster block order).
 * tests/test_gpu_bc7_rot_tasks.py checks it against the exact value in float64: never above it, and not uselessly below. */
void itwTestBc7RotationBounds(const rgba_surface* d_src, float* d_out);

/* The modes 0/2 scan's two cache programs (csrc/bc7.hip search_02, csrc/bc7_f02_schedule.h; tests/test_gpu_bc7_f02_cache.py): for every 4x4
 * block of the device-resident RGBA8 surface the scan runs twice, order 0 = the scheduled visiting order with both caches (what the head scan
 * runs), order 1 = table order with nothing cached.  d_out[(block * 2 + order) * 84 + k] (device memory, raster block order):
 * k = 0, 1 mode 0's winner (error, shape 64..79); 2, 3 mode 2's winner (error, shape 64..127); 4..19 mode 0's error of the shapes with table
 * index 0..15; 20..83 mode 2's error of the shapes with table index 0..63. */
void itwTestBc7F02Scan(const rgba_surface* d_src, int32_t* d_out);

/* BC4 / BC5 (tests/test_gpu_parity_bc4_bc5.py).  The encoders evaluate FindClosestUNORM (BC4BC5.cpp:314-337) through a table
 * the current device builds once by running that search, as written, for all 65 536 endpoint pairs: per pair the 7 texel
 * codes where the chosen index changes and the 8 indices of the runs in between (csrc/bc4_bc5.hip).  Copies the table --
 * 65 536 entries x 4 words {256 - start of run 1..4, one byte each; the same for runs 5..7 with the number of runs in
 * the top byte; indices of runs 0..3, one byte each; indices of runs 4..7} -- to host memory.  Returns 0, or -1 on failure (error mode "return"). */
int itwTestBc45IndexTable(uint32_t* host_out);

/* BC4_SNORM / BC5_SNORM (tests/test_gpu_bc45_snorm.py).  Runs the device function the signed encoders choose their indices with
 * (csrc/bc4_bc5.hip closest_indices_snorm: the run table, and for the endpoint pairs whose entry says "more than 8 runs" the search as
 * written) for all 65 536 endpoint pairs x 256 texel codes: host_out[(r0 << 8 | r1) * 256 + code], r0, r1 and code the int8 values as
 * bytes, 16 MiB of host memory.  Returns 0, or -1 on failure (error mode "return"). */
int itwTestBc45ClosestS(uint8_t* host_out);

/* Which loaders a BC1 / BC3 / BC4 / BC5 call takes (csrc/offset32_host.hpp; tests/test_gpu_large_offsets.py, tests/test_offset32_cpu.py):
 * 1 when the launcher walks a surface of this stride, width and height with 32-bit byte offsets, 0 when it forms 64-bit row addresses.
 * kind 1: BC1, 3: BC3; 4, 8, 16: the BC4 / BC5 family by the bytes of a source texel (4: every RGBA8 source, 8 / 16: the half and float
 * sources of itwCompressNormalMapBC5S).  -1 for any other kind.  The function the launchers call; host arithmetic only. */
int itwTestWalks32(int kind, int64_t stride, int width, int height);

/* Multi-GPU (tests/test_gpu_multigpu_cpp.py): the NEXT itwCompressImageMultiGPU[Ex] call of this process fails inside rank `rank` at `stage`
 * (1 = while preparing, before any transfer is posted; 2 = after its first half-band was posted; 3 = the rank stalls for
 * `stall_ms` before posting anything, which is what the watchdog is for).  One-shot; nothing in the environment can set it. */
void itwMultiGpuTestInjectFailure(int rank, int stage, int stall_ms);

/* The call combiner (csrc/abi.hip coalesce_small_call; tests/test_gpu_call_combiner.py).  One-shot, for the calling thread's current device:
 * the next leader of that device's combiner, before it takes the queue, waits -- without the mutex, like the burst wait, and in its place --
 * until at least `requests` requests are queued or `timeout_ms` have passed.  With `requests` = the number of calling threads all of them
 * reach one batch, whatever their arrival times; with fewer the burst is handed from leader to leader. */
void itwTestCombinerHold(int requests, int timeout_ms);
/* out[0..4] = bursts, batches (leader rounds), requests, merged calls run, holds that ended by their timeout: of this library instance, all
 * devices, since it was loaded.  The hooks build counts always, not only under ITW_COALESCE_DEBUG. */
void itwTestCombinerCounters(int64_t out[5]);

/* The route witness (csrc/bc7.hip launch_bc7, csrc/abi.hip launch(); tests/test_gpu_launch_switches.py): which launch shape the BC7 calls of
 * this library instance took.  Host-side counters only -- no kernel, launch or workspace differs from the product's.
 *   the branch launch_bc7 took, one count per call:        WIDE .. PROBE_IGNORED (the early return for a probe without an order verdict)
 *   inside the bounded routes, one count per call where it holds:
 *     TWO_BANDS     launch_rgb_bounded / launch_alpha_first_bounded7 cut the surface into two bands
 *     PILOT         both gated continuations were enqueued behind the pilot's estimate
 *     PAIRS         the pair route (ITW_BC7_PAIRS)                     ROT_TASKS  the rotation lists (ITW_BC7_ROT_TASKS)
 *     COMPACT       the bands were built with a compact copy of the listed blocks' texels (ITW_BC7_COMPACT)
 *     HOST_VERDICT  the estimate was left for the host (a VERDICT_BAND or PROBE of a staged call)
 *     PROBE         only the estimate ran, nothing was encoded
 *   the LaunchShape::Kind of every BC7 launch() of abi.hip: SHAPE_WHOLE .. SHAPE_PROBE */
enum itw_test_bc7_route {
    ITW_ROUTE_WIDE, ITW_ROUTE_PER_FAMILY, ITW_ROUTE_ALPHA_FIRST_BOUNDED7, ITW_ROUTE_ALPHA_FIRST_BOUNDED, ITW_ROUTE_ALPHA_FIRST_PLAIN,
    ITW_ROUTE_RGB_BOUNDED, ITW_ROUTE_REFERENCE_ORDER, ITW_ROUTE_PROBE_IGNORED,
    ITW_ROUTE_TWO_BANDS, ITW_ROUTE_PILOT, ITW_ROUTE_PAIRS, ITW_ROUTE_ROT_TASKS, ITW_ROUTE_COMPACT, ITW_ROUTE_HOST_VERDICT, ITW_ROUTE_PROBE,
    ITW_ROUTE_SHAPE_WHOLE, ITW_ROUTE_SHAPE_STAGED, ITW_ROUTE_SHAPE_BAND, ITW_ROUTE_SHAPE_VERDICT_BAND, ITW_ROUTE_SHAPE_PROBE,
    ITW_ROUTE_COUNTERS
};
/* out[0 .. min(n, ITW_ROUTE_COUNTERS) - 1] = the counters in the enum's order: of this library instance, all threads and devices, since it was
 * loaded or last reset. */
void itwTestBc7RouteCounters(int64_t* out, int n);
void itwTestBc7RouteCountersReset(void);

/* What a two-band call of the RGB bounded order counted on the device.  Arm (on != 0), run calls, read: each such call synchronises and leaves
 * its counters, the last one stands.  out[0 .. min(n, ITW_BC7_CALL_COUNTERS) - 1] in the enum's order; the per-band ones are band 0 then band 1. */
enum itw_test_bc7_call_counter {
    ITW_BC7_CC_PILOT_LISTED, ITW_BC7_CC_PILOT_SAMPLED, ITW_BC7_CC_PILOT_FLAG,
    ITW_BC7_CC_ROT_LISTS,                               /* [2][3]: the rotation lists' lengths */
    ITW_BC7_CC_LISTED = ITW_BC7_CC_ROT_LISTS + 6,       /* [2]: blocks listed for modes 1/3 */
    ITW_BC7_CC_PAIRS = ITW_BC7_CC_LISTED + 2,           /* [2]: (block, shape) pairs in the buckets */
    ITW_BC7_CC_OVERFLOW = ITW_BC7_CC_PAIRS + 2,         /* [2]: a bucket overflowed */
    ITW_BC7_CC_REDO = ITW_BC7_CC_OVERFLOW + 2,          /* [2]: blocks deferred to the full list scan */
    ITW_BC7_CALL_COUNTERS = ITW_BC7_CC_REDO + 2
};
void itwTestBc7CallCountersArm(int on);
void itwTestBc7CallCounters(int32_t* out, int n);

/* The sRGB mip filter's encode on the device (csrc/mipgen.hpp mip_srgb_encode, the function the mip kernels store R, G, B with under
 * ITW_MIP_SRGB): d_out[i] = E(d_in[i]) for `n` floats resident in device memory, on the calling thread's stream.
 * tests/test_gpu_srgb_mips.py compares it with the counting definition of include/itw_dispatch.h around every threshold. */
void itwTestSrgbEncode(const float* d_in, uint8_t* d_out, int64_t n);

/* Which alpha histogram kernel the coverage rule and itwAlphaCoverage launch (csrc/mip_alpha.hip): 0, the product's, takes one
 * LDS atomic per texel for every bin; 1 counts the 0 and 255 bins per wave (ballot + popcount).  Both give the same counts; tools/alpha_mip_timing.py times them against
 * each other and tests/test_gpu_alpha_mips.py compares their output.  Process-wide. */
void itwTestAlphaHistVariant(int spikes);

/* Which cubic mip kernel ITW_MIP_CUBIC launches (csrc/mip_filters.hip): 0 reads its 16 taps from memory, 1 stages the workgroup's source
 * window in LDS first.  Both write the same bytes; tools/mip_filter_timing.py times them against each other and
 * tests/test_gpu_mip_filters.py runs both.  Process-wide; the product's choice is the library's default. */
void itwTestMipCubicVariant(int lds);

/* The host's per-axis tables of the cubic and triangle mip filters (csrc/mip_filters.hpp), as tests/golden/mipfilter_ref.npz records the
 * reference's _CreateCubicFilter and TriangleFilter::_Create.  kind 1, cubic: index[4 * u .. 4 * u + 3] = the four taps of destination u,
 * weight[u] = its x; returns dest.  kind 2, triangle: entry e in the reference's stored order, index[2 * e] = the source texel,
 * index[2 * e + 1] = the destination, weight[e] = the weight; returns the number of entries.  `capacity` counts destinations (cubic) or
 * entries (triangle) the arrays hold; -1 when it is too small or an argument is out of range.  Host arithmetic only. */
int64_t itwTestMipFilterTable(int kind, int source, int dest, int wrap, int32_t* index, float* weight, int64_t capacity);

/* The host's per-axis tables of the free-size chain (ITW_MIP_RESIZE; csrc/mip_filters.hpp), the functions csrc/resize.hip's kernels run, as
 * tests/golden/resize_ref.npz records the reference's.  `address`: 0 clamp, 1 wrap, 2 mirror.  kind 1, cubic: as itwTestMipFilterTable's,
 * under any addressing.  kind 3, point: index[u] = the source texel of destination u, weight[u] = 1.  kind 4, linear
 * (_CreateLinearFilter as written, wrap branches included; mirror is clamp): index[2 * u], index[2 * u + 1] = u0, u1 and
 * weight[2 * u], weight[2 * u + 1] = weight0, weight1.  Returns dest; -1 when `capacity` (destinations) is below dest or an argument is
 * out of range.  The triangle lists of any pair are itwTestMipFilterTable's.  Host arithmetic only. */
int64_t itwTestResizeTable(int kind, int source, int dest, int address, int32_t* index, float* weight, int64_t capacity);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
