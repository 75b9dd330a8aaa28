// kernels.hpp -- host-visible launchers of the gfx950 encoder kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ispc_texcomp.h"

namespace itw {

// All launchers: `src`/`dst` are DEVICE pointers, rows `stride` bytes apart,
// output tightly packed in raster block order; asynchronous on `st`.
void launch_bc1 (const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, hipStream_t st);
void launch_bc3 (const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, hipStream_t st);
// ETC1 of the RGB channels of an RGBA8 surface (etc1.hip): (width / 4) * (height / 4) blocks of 8 bytes; `threshold` >= 1 (fastSkipTreshold,
// anything above 165 is 165); src and stride 4-byte aligned.  One launch, no workspace.
void launch_etc1(const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, int threshold, hipStream_t st);
// BC4_UNORM / BC5_UNORM of the R (and G) channel of an RGBA8 surface, DirectXTex's encoder (bc4_bc5.hip).  Any
// width/height >= 1: ceil(width/4) x ceil(height/4) blocks, partial blocks replicated by DirectXTex's rule.
void launch_bc4 (const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, hipStream_t st);
void launch_bc5 (const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, hipStream_t st);
// BC1 with 1-bit alpha of an RGBA8 surface, DirectXTex's D3DXEncodeBC1 (bc1a.hip): ceil(width/4) x ceil(height/4) blocks of 8 bytes, partial
// blocks filled as BC4 / BC5's; a texel is transparent when its alpha < alpha_ref; `flags`: ITW_BC_* (itw_dispatch.h).  src and stride 4-byte aligned.
void launch_bc1a(const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, float alpha_ref, uint32_t flags, hipStream_t st);
// BC2 of an RGBA8 surface, DirectXTex's D3DXEncodeBC2 (bc2.hip): ceil(width/4) x ceil(height/4) blocks of 16 bytes, partial blocks filled as
// BC4 / BC5's; `flags`: ITW_BC_* (itw_dispatch.h).  src and stride 4-byte aligned, dst 16-byte aligned.
void launch_bc2(const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, uint32_t flags, hipStream_t st);
// BC3 of an RGBA8 surface by DirectXTex's D3DXEncodeBC3 (bc3_dxtex.hip; launch_bc3 above is kernel.ispc's encoder): ceil(width/4) x ceil(height/4)
// blocks of 16 bytes, partial blocks filled as BC4 / BC5's; `flags`: ITW_BC_* (itw_dispatch.h).  src, stride and dst 4-byte aligned.
void launch_bc3_dxtex(const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, uint32_t flags, hipStream_t st);
void launch_bc4s(const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, hipStream_t st);   // BC4_SNORM / BC5_SNORM of an RGBA8_SNORM surface
void launch_bc5s(const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, hipStream_t st);
// BC5_UNORM of a normal map: the stages `ops` (ITW_NORMAL_*, 1..7; normal_prep.hpp) applied to the texels as the kernel loads them
void launch_bc5_normal(const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst, uint32_t ops, hipStream_t st);
// BC5_SNORM of a signed normal source (normal_prep.hpp): texel_bytes 4 (RGBA8_SNORM), 8 (RGBA16F) or 16 (RGBA32F), src and stride 4-byte aligned,
// the stages `ops` (0..7) and the quantisation applied as the kernel loads the texels; (4, ops 0) is launch_bc5s
void launch_bc5s_normal(const uint8_t* src, int texel_bytes, int64_t stride, int width, int height, uint8_t* dst, uint32_t ops, hipStream_t st);
void warmup_bc45s();                                            // the same for the SNORM encoders' table (FindClosestSNORM)
void copy_bc45_closest_snorm(uint8_t* host_out, hipStream_t st);  // test hook: the SNORM encoders' index for every (endpoint pair, code), 16 MiB
void warmup_bc45();                                               // builds the current device's FindClosestUNORM run table now (else: first call)
void copy_bc45_index_table(uint32_t* host_out, hipStream_t st);   // test hook: the FindClosestUNORM run table of the current device
// which surfaces launch_bc1 / launch_bc3 (bc3) and launch_bc4 .. launch_bc5s_normal (texel_bytes: 4 for RGBA8) walk with 32-bit byte offsets:
// offset32_host.hpp's rule with each launcher's block row and output.  A pure function of these arguments.
bool bc13_walks_32(bool bc3, int64_t stride, int width, int height);
bool bc45_walks_32(int texel_bytes, int64_t stride, int width, int height);
// BC7 runs as up to seven kernels (search + finish per multi-subset mode family, one for modes 4/5/6) that hand
// "best error so far" and the search winners to each other through
// `workspace`: device memory, bc7_workspace_bytes(width, height) bytes, 16 B aligned, contents irrelevant on entry.
// `settings` (optional): size for what a call with these settings can touch -- the lists, band regions and compact texel copy belong to the
// alpha-first and bounded mode orders (36 B per block without them, ~124 with); nullptr sizes for any settings.
size_t bc7_workspace_bytes(int width, int height, int64_t wide_max_blocks = 0, const bc7_enc_settings* settings = nullptr);   // wide_max_blocks as in Bc7Aux
// BC7 launch shape: 0 = by call size (default), 1 = deep (one lane per block, a launch pair per mode family: fills the
// chip on whole surfaces), 2 = wide (split scans + ordered argmin: small calls).  Same blocks either way.
void set_bc7_path(int path);
bool bc7_scans_every_shape(const bc7_enc_settings& s);  // the settings take the bounded mode order (modes 1/3 -- and 7 -- scan all 64 shapes: `slow`, `alpha_slow`): about twice the work per block
bool bc7_has_order_verdict(const bc7_enc_settings& s);   // the settings run the bounded order of the RGB profiles (the one with a pilot's estimate)
bool bc7_staged_bands_ok();      // the staged runs of a host-pointer call may run as overlapped deep bands (not when the wide shape is forced / ITW_STAGED_BANDS=0)
// The pilot of the bounded BC7 mode order (bc7.hip, launch_bc7): percent of the blocks the pilot looks at that its estimate may list for modes 1/3 for the rest of
// the surface to take the bounded order; -1 = no pilot, the whole call in the bounded order.  Same blocks whatever the value.
void set_bc7_pilot(int percent);
// `aux` (optional): a second stream of the same device plus two events the launcher may use to run independent parts of a
// small call side by side; everything is joined back into `st` before the launcher returns.
// `mid` (may be null: no pilot): a third event, for the pilot of the bounded mode order (bc7.hip).  `single`: the call is one band of a
// larger job whose bands the CALLER overlaps on two streams (the staged runs of a host-pointer call, abi.hip): deep shape whatever the
// size, everything on `st`, no pilot, no inner bands.
// `verdict` (optional, `single` calls): where a call that runs the bounded order leaves the pilot's estimate for the HOST -- {blocks some
// two-subset shape can still improve, blocks looked at}, written by the estimate kernel's last workgroup straight into PINNED HOST memory
// (`host_counts_dev` = the device-side address of the caller's two pinned words, `host_counts` = their host address), complete once `event`
// (recorded behind that kernel) has fired: the host reads two words, no copy on any stream.  The caller of the first staged run polls it
// under the upload of the next run and picks the launch shape of the remaining runs (abi.hip).
struct Bc7Verdict { hipEvent_t event; volatile int32_t* host_counts; bool valid; int32_t* host_counts_dev; };
// `probe` (with `single` and `verdict`): only the pilot's estimate is computed -- the {0,2} scan of every eighth chunk and the count -- nothing
// is encoded (a staged call whose runs take the wide shape keeps its verdict fresh this way).
struct Bc7Aux { hipStream_t stream; hipEvent_t fork, join; int64_t wide_max_blocks; hipEvent_t mid; bool single; Bc7Verdict* verdict; bool probe; };   // wide_max_blocks: 0 = the library default
void launch_bc7 (const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst,
                 const bc7_enc_settings& s, float* workspace, hipStream_t st, const Bc7Aux* aux = nullptr);
// test hook: bc7_exact.hpp's two_subset_bound of all 64 two-subset shapes of every block, out[block * 64 + shape] (device memory)
void launch_bc7_test_bounds(const uint8_t* src, int64_t stride, int width, int height, float* out, hipStream_t st);
void launch_bc7_test_rot_bounds(const uint8_t* src, int64_t stride, int width, int height, float* out, hipStream_t st);
void launch_bc7_test_f02_scan(const uint8_t* src, int64_t stride, int width, int height, int32_t* out, hipStream_t st);
// test hook (itwTestBc7RouteCounters): the route witness, host-side counters indexed by include/itw_test_hooks.h's itw_test_bc7_route.  The hooks build
// counts one at ITW_ROUTE_SEEN(what); in the product the macro is empty.
#ifdef ITW_TEST_HOOKS
void bc7_route_seen(int what);
void bc7_route_counters(int64_t* out, int n);
void bc7_route_counters_reset();
void bc7_arm_call_counters(int on);                      // test hook (itwTestBc7CallCounters): two-band RGB bounded calls leave their device counters
void bc7_call_counters(int32_t* out, int n);
#define ITW_ROUTE_SEEN(what) ::itw::bc7_route_seen(what)
#else
#define ITW_ROUTE_SEEN(what) ((void)0)
#endif
// `workspace`: device memory of bc6h_workspace_bytes(width, height, s) bytes (0 for most calls: only small calls of the slow
// profiles, which take the wide shape, need any); nullptr keeps the one-kernel path.
size_t bc6h_workspace_bytes(int width, int height, const bc6h_enc_settings& s);
void launch_bc6h(const uint8_t* src, int64_t stride, int width, int height, uint8_t* dst,
                 const bc6h_enc_settings& s, hipStream_t st, void* workspace = nullptr);
void set_bc6h_path(int path);         // 0 by size, 1 one kernel, 2 wide (tests / probes)

// DirectXTex's partial-block fill (DirectXTexCompress.cpp:140-168 applied in its own order): texel column / row i of a block of which
// only the first `valid` (1..4) columns / rows exist repeats source column / row {0,0,0,1}[i], itself wrapped to 0 when that one is
// missing too.  Shared by the BC4/BC5 kernel's load (bc4_bc5.hip) and the chain gather (chain.hip).
__device__ __forceinline__ int bc45_fill_index(int i, int valid)
{
    const int s = i < valid ? i : (i == 3 ? 1 : 0);
    return s < valid ? s : 0;
}

// One image of a chain (chain.hip): texels at `ptr` (device memory), rows `stride` bytes apart, width x height >= 1, and the index of its
// first block in its group's concatenated block list (ceil(w/4) x ceil(h/4) blocks per image, raster order).
struct ChainImage { const uint8_t* ptr; int64_t stride; int32_t width, height; int64_t first_block; };
// The gather of one group of a chain into a PACKED surface: `packed_bx` blocks wide, `packed_by` block rows high (4 * packed_bx texels x
// 4 * packed_by rows, `dst_pitch` bytes apart, 16-B aligned rows), packed block j = block j of the group (j < nblocks; the tail of the last
// packed row is zero).  `images`: device table of `nimg` descriptors, ascending first_block.  texel_bytes 4 (RGBA8) or 8 (RGBA16F);
// `fill45`: partial blocks take bc45_fill_index (BC4/BC5) instead of edge replication (the ISPC formats' pad to multiples of 4).
// `extents` (optional, edge replication only): device memory, one byte per block j < nblocks: (pw - 1) | (ph - 1) << 2, the pw x ph texels
// of the block that lie inside its image.  `normal_ops` (ITW_NORMAL_*, itw_dispatch.h; not with `extents`): the normal-map stages applied
// to every texel as it is copied (normal_prep.hpp).  `signed_source` (4, 8 or 16; texel_bytes 4 and fill45 only): the images are signed
// normal sources of that many bytes per texel and `normal_ops` (0..7) has its signed meaning: each texel is quantised to its RGBA8_SNORM word
// as it is copied.
void launch_chain_gather(const ChainImage* images, int nimg, int64_t nblocks, int packed_bx, int packed_by, int texel_bytes, bool fill45,
                         uint8_t* dst, int64_t dst_pitch, hipStream_t st, uint8_t* extents = nullptr, uint32_t normal_ops = 0, int signed_source = 0);

// Height maps to normal maps (height_normal.hip; the `ops` word with ITW_NORMAL_FROM_HEIGHT, itw_dispatch.h).
// One image of a call: heights at `src`, the normal map at `dst` (device memory, disjoint), rows `*_stride` bytes apart, and the index of
// its first work unit in the call's list: height_units() each, tiles of 64 x 16 texels.  height_units_fit: one launch covers a list of
// that many.
int64_t height_units(int width, int height);
bool height_units_fit(int64_t units);
struct HeightLevel { const uint8_t* src; uint8_t* dst; int64_t src_stride, dst_stride; int32_t width, height; int64_t first_unit; };
// One launch over `count` images: `d_levels` their device table (unused for one image, which travels as `first`), `units` the list's
// length; the kinds are hn::Src / hn::Dst of height_normal_core.hpp.  Bits 0..2 of `ops` apply after the stage, in registers.
void launch_height_normal(int src_kind, int dst_kind, const HeightLevel* d_levels, const HeightLevel& first, int count, int64_t units, uint32_t ops, hipStream_t st);
int height_signed_source_kind(int texel_bytes);                  // hn::Src of a signed normal source of 4, 8 or 16 bytes per texel
// An `ops` word as `who`'s failure when it is not one: unknown bits, a channel above 5, amplitude bits that are no finite half above 0, or --
// `no_height` given -- ITW_NORMAL_FROM_HEIGHT on a call that cannot take it, with `no_height` as the reason.  normal_ops_fault: the same
// verdict without a message.
void check_normal_ops(const char* who, uint32_t ops, const char* no_height = nullptr);
bool normal_ops_fault(uint32_t ops);
// the stage from one base (device memory) into level 0 of a device-side chain: one launch
void height_level0(int src_kind, int dst_kind, const uint8_t* src, int64_t src_stride, const rgba_surface& level0, uint32_t ops, hipStream_t st);
// no target may overlap a source's bytes (itwQuantizeNormalMapChain with ITW_NORMAL_FROM_HEIGHT): a failure otherwise
void height_check_disjoint(const char* who, const rgba_surface* sources, int texel_bytes, const rgba_surface* targets, int count);
// the device work of itwPrepareNormalMapChain / itwQuantizeNormalMapChain with ITW_NORMAL_FROM_HEIGHT: images that passed the checks
void height_prepare_chain(const rgba_surface* images, int count, int pixel_size, uint32_t ops, bool dev);
void height_quantize_chain(const rgba_surface* sources, int texel_bytes, const rgba_surface* targets, int count, uint32_t ops, bool dev);

} // namespace itw
