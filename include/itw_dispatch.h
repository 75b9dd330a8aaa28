/*
 * itw_dispatch.h -- portable restatement of the reference's threading / dispatch layer
 * (3rdParty/Intel/Source/win32Threads.h:24-80, win32Threads.cpp:98-329): the immediate caller of the
 * CompressBlocks* C ABI.  Same entry points, same argument meaning; Win32 types replaced by portable ones
 * (BYTE -> uint8_t, DXGI_FORMAT -> int carrying the DXGI_FORMAT_* value) and C linkage, so any host language can
 * bind it.
 *
 * What changes underneath: the reference keeps a pool of up to 64 Win32 threads and hands each a 4-row-aligned band
 * of the surface (win32Threads.cpp:211-249).  Here a "worker" is a GPU: CompressImageMT cuts the surface with the
 * same band rule over GetProcessorCount() = number of visible MI355X devices and runs one band per device from a
 * persistent pool of host threads (one per device), so a single-GPU box makes ONE whole-surface call instead of
 * dozens of few-thousand-pixel calls, and an 8-GPU node encodes 8 bands concurrently in one process.
 */
#ifndef ITW_DISPATCH_H
#define ITW_DISPATCH_H

#include <stddef.h>
#include "ispc_texcomp.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)   /* the library is built with -fvisibility=hidden: only what the headers declare is exported */

/* win32Threads.h:24 */
typedef void (CompressionFunc)(const rgba_surface* input, uint8_t* output);

/* the DXGI_FORMAT values the dispatch layer understands (dxgiformat.h; win32Threads.cpp:192-209) */
enum {
    ITW_DXGI_FORMAT_BC1_UNORM = 71, ITW_DXGI_FORMAT_BC1_UNORM_SRGB = 72,
    ITW_DXGI_FORMAT_BC3_UNORM = 77, ITW_DXGI_FORMAT_BC3_UNORM_SRGB = 78,
    ITW_DXGI_FORMAT_BC4_UNORM = 80, ITW_DXGI_FORMAT_BC5_UNORM = 83,       /* the DirectXTex formats, itw_bc45.h */
    ITW_DXGI_FORMAT_BC4_SNORM = 81, ITW_DXGI_FORMAT_BC5_SNORM = 84,       /* their signed pair (RGBA8_SNORM sources), itw_bc45.h */
    ITW_DXGI_FORMAT_BC6H_UF16 = 95, ITW_DXGI_FORMAT_BC6H_SF16 = 96,
    ITW_DXGI_FORMAT_BC7_UNORM = 98, ITW_DXGI_FORMAT_BC7_UNORM_SRGB = 99,
    /* ETC1 has no DXGI code: it goes by its GL enum, GL_ETC1_RGB8_OES (also KTX's glInternalFormat: itwKtx*, itw_dds.h).  Taken by the decode and
     * measure entry points of itw_decode.h and, with `settings` = const etc_enc_settings*, by itwCompressImageSlicedEx, itwSliceWindow[For],
     * itwChainBytes and itwCompressImageChain[Ex] below (the block encoder is itwCompressBlocksETC1, itw_amd.h).  It has no CompressImage*
     * trampoline, so itwCompressImageSliced / itwCompressImageChain run a caller's function as the literal loop; the refined calls, the
     * multi-GPU calls and DDS do not know it. */
    ITW_FORMAT_ETC1_RGB8 = 0x8D64,
    /* BC1 with 1-bit alpha (punch-through, "DXT1A"): DirectXTex's colour-key encoder, D3DXEncodeBC1 (BC.cpp) as DirectX::Compress calls it.
     * DXGI has no code of its own for it, GL has: GL_COMPRESSED_RGBA_S3TC_DXT1_EXT and GL_COMPRESSED_SRGB_ALPHA_S3TC_DXT1_EXT (the second
     * only labels the stream, like 72).  The stream IS a BC1 stream: the decode, measure and preview entry points of itw_decode.h take the
     * two codes as synonyms of 71 / 72, itwDds* writes them with the header of 71 / 72 (a file read back says 71 / 72); KTX does not know them.
     * Encoded, with `settings` = const itw_bc1a_settings* or NULL (below), by itwCompressImageSlicedEx (one slice is the single-image call),
     * itwCompressImageChainEx and the itwCompressImageMipped* calls; itwSliceWindow[For], itwChainBytes and GetBytesPerBlock (8) know them.
     * They are DirectXTex formats (itw_bc45.h): an RGBA8 source of any size >= 1, partial blocks kept and filled by DirectXTexCompress.cpp's
     * {0, 0, 0, 1} rule.  A texel code v is the float (float)v * (1.0f / 255.0f).  There is no block-level entry point and no CompressImage*
     * trampoline: itwCompressImageSliced / itwCompressImageChain run a caller's function as the literal loop, CompressImageMT / ST have no
     * function to call; the refined calls, the multi-GPU calls and the normal-map chain calls refuse the codes.  BC2 is the two codes below. */
    ITW_FORMAT_BC1A_UNORM = 0x83F1, ITW_FORMAT_BC1A_UNORM_SRGB = 0x8C4D,
    /* BC2 (DXT2 / DXT3: 4 bits of explicit alpha per texel beside a four-colour BC1 block, 16 bytes per block): DirectXTex's D3DXEncodeBC2
     * (BC.cpp) as DirectX::Compress calls it.  It goes by its GL enums, GL_COMPRESSED_RGBA_S3TC_DXT3_EXT and
     * GL_COMPRESSED_SRGB_ALPHA_S3TC_DXT3_EXT (the second only labels the stream, like 72): DXGI 74 / 75 stay refused codes at every entry
     * point that takes a format code, and appear only inside DDS descriptors and headers (itw_dds.h), where they are the file's own truth.
     * Encoded, with `settings` = const itw_bc1a_settings* or NULL (below), by itwCompressImageSlicedEx (one slice is the single-image call),
     * itwCompressImageChainEx and the itwCompressImageMipped* calls (ITW_MIP_SRGB, the filter and wrap bits, weight_colour and coverage_ref
     * apply: the texels are RGBA8 colour); itwSliceWindow[For], itwChainBytes and GetBytesPerBlock (16) know the codes.  Decoded, measured
     * and previewed by the entry points of itw_decode.h under the same two codes.  A DirectXTex format like BC1A: any size >= 1, partial
     * blocks kept and filled by the {0, 0, 0, 1} rule, the same texel conversion, no block-level entry point and no CompressImage* trampoline
     * (itwCompressImageSliced / itwCompressImageChain run a caller's function as the literal loop); the refined calls, the multi-GPU calls,
     * the normal-map chain calls, any normal_ops and KTX refuse the codes. */
    ITW_FORMAT_BC2_UNORM = 0x83F2, ITW_FORMAT_BC2_UNORM_SRGB = 0x8C4E,
    /* BC3 (DXT4 / DXT5) by DirectXTex's encoder, D3DXEncodeBC3 (BC.cpp) as DirectX::Compress calls it -- what `texconv -f DXT5 [-bcdither]
     * [-bcuniform]` writes, byte for byte -- beside kernel.ispc's CompressBlocksBC3, which stays the encoder of DXGI 77 / 78 at every entry
     * point.  The codes are the GL enums GL_COMPRESSED_RGBA_S3TC_DXT5_EXT and GL_COMPRESSED_SRGB_ALPHA_S3TC_DXT5_EXT (the second only labels
     * the stream, like 78).  The stream IS a BC3 stream: the decode, measure and preview entry points of itw_decode.h take the two codes as
     * synonyms of 77 / 78, itwDds* writes them with the header of 77 / 78 (a file read back says 77 / 78); KTX does not know them.
     * Encoded, with `settings` = const itw_bc1a_settings* or NULL (below), by itwCompressImageSlicedEx (one slice is the single-image call),
     * itwCompressImageChainEx and the itwCompressImageMipped* calls (ITW_MIP_SRGB, the filter, wrap and resize bits, weight_colour and
     * coverage_ref apply: the texels are RGBA8 colour); itwSliceWindow[For], itwChainBytes and GetBytesPerBlock (16) know the codes.  A
     * DirectXTex format like BC1A and BC2: any size >= 1, partial blocks kept and filled by the {0, 0, 0, 1} rule, the same texel conversion,
     * no block-level entry point and no CompressImage* trampoline (itwCompressImageSliced / itwCompressImageChain run a caller's function as
     * the literal loop); the refined calls, the multi-GPU calls, the normal-map chain calls, any normal_ops and KTX refuse the codes. */
    ITW_FORMAT_BC3_DXTEX = 0x83F3, ITW_FORMAT_BC3_DXTEX_SRGB = 0x8C4F,
    /* The SIGNED reading of a BC6H stream (what a GPU shows for a texture labelled DXGI_FORMAT_BC6H_SF16; DirectXTex's D3DXDecodeBC6HS), by its
     * GL enum, GL_COMPRESSED_RGB_BPTC_SIGNED_FLOAT.  A DECODE code only: itwDecodeBlocks, itwDecodeChain, itwDecodeImage, itwMeasureBlocks,
     * itwMeasureChain and itwPreviewBlocks take it (itw_decode.h).  DXGI 96 keeps every meaning it has at each entry point (the encoder
     * writes the reference's unsigned-coded blocks under it, itwDecodeBlocks reads it as unsigned, the chain and preview calls refuse it).
     * There is no signed BC6H encoder: every call that encodes -- itwCompressImageSlicedEx, itwCompressImageChain[Ex], the mipped, refined,
     * normal-map and multi-GPU calls -- fails through the error mode before any device work with a message that says so; itwChainBytes
     * returns -1, itwSliceWindow[For] 0, GetBytesPerBlock 16 (the stream's block size).  It is not a descriptor code:
     * itwDds* return 0 for it (a file's header says 96, and itwDdsReadHeader reports 96); KTX does not know it. */
    ITW_FORMAT_BC6H_SIGNED = 0x8E8E
};

/* Settings of the two BC1A codes and of the two BC2 codes.  flags: DirectXTex's BC_FLAGS_* values (BC.h) -- error diffusion of the colours, of alpha (the key test
 * then sees the diffused, rounded alpha, not the source's), uniform instead of perceptual channel weights.
 * NULL settings mean alpha_ref = 0.5f, flags = 0: TEX_THRESHOLD_DEFAULT, what the plugin passes to DirectX::Compress.  The struct is copied
 * while the call is set up.  A struct_size other than 16, reserved != 0, unknown flag bits or a non-finite alpha_ref fail the call through
 * the error mode before any device work.  Any finite alpha_ref behaves as the reference does: a texel is transparent when its alpha
 * (float) < alpha_ref, so <= 0 makes no texel transparent and > 1 makes every block 00 00 FF FF FF FF FF FF.
 * A caller who kept alpha-test coverage with coverage_ref = r (itwCompressImageMippedAlpha) passes alpha_ref = (float)r * (1.0f / 255.0f):
 * that is the texel conversion's own expression, so "transparent" is exactly a < r on the integer codes.
 * BC2: the same struct and the same checks.  alpha_ref is checked (finite) but not read -- BC2 has no colour key: D3DXEncodeBC2 calls
 * EncodeBC1(bColorKey = false), always four colours; ITW_BC_DITHER_A diffuses the error of the 4-bit alpha; NULL means flags 0.
 * The two BC3_DXTEX codes: the same struct and the same checks, alpha_ref checked (finite) but not read like BC2's.  ITW_BC_DITHER_A diffuses
 * the error of the 3-bit alpha indices inside the block (D3DXEncodeBC3 also diffuses where it rounds alpha to 8 bits before it chooses the
 * endpoints; an RGBA8 source leaves nothing to diffuse there); ITW_BC_DITHER_RGB and ITW_BC_UNIFORM act on the colour half. */
enum { ITW_BC_DITHER_RGB = 0x10000, ITW_BC_DITHER_A = 0x20000, ITW_BC_UNIFORM = 0x40000 };
typedef struct itw_bc1a_settings { uint32_t struct_size /* 16 */; float alpha_ref; uint32_t flags, reserved /* 0 */; } itw_bc1a_settings;

/* win32Threads.h:52-55 / win32Threads.cpp:98-190.  GetProcessorCount(): number of workers = visible GPUs (>= 1), or the
 * value of the environment variable ITW_WORKERS when set (extra workers share the devices round-robin).
 * InitWin32Threads() starts the pool (idempotent); DestroyThreads() joins it.  CompressImageMT initialises lazily. */
int  GetProcessorCount(void);
void InitWin32Threads(void);
void DestroyThreads(void);

/* win32Threads.cpp:192-209: 8 for BC1 (and anything unknown, so BC4 and BC4_SNORM too), 16 for BC3 / BC7 / BC6H -- and for BC5 and
 * BC5_SNORM, which the reference's switch does not list because BC5 never reaches it there */
int  GetBytesPerBlock(int dxgi_format);

/* win32Threads.cpp:211-249, 277-282.  `input`/`output` are host or device pointers exactly as CompressBlocks* accepts
 * them (device pointers must be reachable from every GPU that takes a band, i.e. single-GPU or managed memory).
 * Blocks until the whole surface is encoded; returns true like the reference. */
bool CompressImageMT(const rgba_surface* input, uint8_t* output, CompressionFunc* cmpFunc, int dxgi_format);
bool CompressImageST(const rgba_surface* input, uint8_t* output, CompressionFunc* cmpFunc, int dxgi_format);

/* win32Threads.h:58-80 / win32Threads.cpp:289-329: profile trampolines */
void CompressImageBC1(const rgba_surface* input, uint8_t* output);
void CompressImageBC3(const rgba_surface* input, uint8_t* output);
/* same shape for the two formats the plugin sends to DirectX::Compress instead (IntelPlugin.cpp:271-273); with these the
 * band / slice rules above also keep the partial last block row and column (itw_bc45.h) */
void CompressImageBC4(const rgba_surface* input, uint8_t* output);
void CompressImageBC5(const rgba_surface* input, uint8_t* output);
void CompressImageBC4S(const rgba_surface* input, uint8_t* output);     /* ITW_DXGI_FORMAT_BC4_SNORM / BC5_SNORM: CompressBlocksBC4S / BC5S */
void CompressImageBC5S(const rgba_surface* input, uint8_t* output);
void CompressImageBC7_ultrafast(const rgba_surface* input, uint8_t* output);
void CompressImageBC7_veryfast(const rgba_surface* input, uint8_t* output);
void CompressImageBC7_fast(const rgba_surface* input, uint8_t* output);
void CompressImageBC7_basic(const rgba_surface* input, uint8_t* output);
void CompressImageBC7_slow(const rgba_surface* input, uint8_t* output);
void CompressImageBC7_alpha_ultrafast(const rgba_surface* input, uint8_t* output);
void CompressImageBC7_alpha_veryfast(const rgba_surface* input, uint8_t* output);
void CompressImageBC7_alpha_fast(const rgba_surface* input, uint8_t* output);
void CompressImageBC7_alpha_basic(const rgba_surface* input, uint8_t* output);
void CompressImageBC7_alpha_slow(const rgba_surface* input, uint8_t* output);
void CompressImageBC6H_veryfast(const rgba_surface* input, uint8_t* output);
void CompressImageBC6H_fast(const rgba_surface* input, uint8_t* output);
void CompressImageBC6H_basic(const rgba_surface* input, uint8_t* output);
void CompressImageBC6H_slow(const rgba_surface* input, uint8_t* output);
void CompressImageBC6H_veryslow(const rgba_surface* input, uint8_t* output);

/* The plugin's slice loop with progress / early out (IntelPlugin.cpp:851-879): the surface is cut into
 * `slices = width*height / slice_pixels` (>= 1) runs of block rows (rows [i*h/slices & ~3, (i+1)*h/slices & ~3), the reference's
 * arithmetic), `progress(i, slices, user)` is called for i = 1 .. slices-1 in order and aborts the job when it returns false (the
 * call then returns false).  `target` is the block array with `block_row_pitch` bytes between block rows (the reference passes the
 * DDS image's rowPitch); slice_pixels <= 0 selects the reference's 0x40000.
 *
 * The reference encodes slice i between progress(i) and progress(i+1), one synchronous CompressImageMT/ST call each.  Here, when
 * `cmpFunc` is one of THIS library's CompressImage* trampolines, the slices run as a PIPELINE instead:
 * W consecutive slices form a window (upload, kernels and download of neighbouring windows overlap on three streams; W =
 * itwSliceWindow(...): about 131 072 blocks, 262 144 for BC1/BC3/BC4/BC5 -- 0.3-1 ms of work, so any job long enough to show a progress bar
 * has many windows), and progress(i) is called once slice i-1 -- and
 * every slice before it -- is in `target`.  What a caller can observe of the difference:
 *   * when progress(i) returns false, slices < i are written like in the reference, and so may be up to W-1 slices after them (the
 *     rest of slice i-1's window); the window being encoded at that moment is drained and NOT copied back -- bytes of `target` behind slice
 *     i-1's window are not written, whether `target` is host or device memory (with `progress` set, a device target receives each window as
 *     it retires instead of being written by the kernels in flight);
 *   * progress calls of one window arrive back to back;
 *   * `progress` runs on the calling thread while later windows are in flight on that thread's streams and staging buffers: it must not
 *     call back into this library on the same thread (Photoshop's SetProgress does not).
 * Several GPUs (`multithreaded` and GetProcessorCount() > 1, host memory): one pipeline PER GPU -- window k runs on worker k % n, each worker
 * on its own device, and the calling thread calls progress(i) once every window up to slice i-1's has arrived, i.e. still in order; on an
 * abort windows other GPUs had already finished further down the image stay written too.
 * Any other `cmpFunc` (a caller's own function: opaque), itwSetSliceWindow(-1) or a single slice: the literal loop.  Host or device
 * pointers; synchronous either way. */
typedef bool (ItwProgressFunc)(int done, int total, void* user);
bool itwCompressImageSliced(const rgba_surface* source, uint8_t* target, int64_t block_row_pitch, CompressionFunc* cmpFunc,
                            int dxgi_format, bool multithreaded, int64_t slice_pixels, ItwProgressFunc* progress, void* user);
/* The pipeline itself, for callers that hold a settings struct rather than a trampoline: `settings` = bc7_enc_settings* (BC7),
 * bc6h_enc_settings* (BC6H), etc_enc_settings* (ITW_FORMAT_ETC1_RGB8: RGBA8 source, alpha ignored, partial blocks dropped, 8-byte blocks;
 * a null pointer or fastSkipTreshold < 1 fails through the error mode before any device work, a threshold above 165 is 165; the threshold
 * is copied, the struct need not outlive the call's setup), ignored otherwise.  Same slices, progress contract and return value. */
bool itwCompressImageSlicedEx(const rgba_surface* source, uint8_t* target, int64_t block_row_pitch, int dxgi_format, const void* settings,
                              int64_t slice_pixels, ItwProgressFunc* progress, void* user);
/* W: slices per window.  itwSetSliceWindow(n > 0) fixes it process-wide (1 = the reference's early-out granularity exactly), 0 = by
 * format and size (default; env ITW_SLICE_WINDOW presets it), n < 0 = no pipeline: itwCompressImageSliced runs the literal loop
 * (also env ITW_SLICED_PIPELINE=0).  itwSliceWindow reports what a call would use (0: the literal loop). */
void itwSetSliceWindow(int slices);
int  itwSliceWindow(int dxgi_format, int width, int height, int64_t slice_pixels);
/* ... for given settings (bc7_enc_settings* / bc6h_enc_settings* / etc_enc_settings* / NULL): ETC1 takes BC7's ~131 072 blocks; BC7 settings whose modes 1/3 scan every two-subset shape (`slow`, `alpha_slow`:
 * twice the work per block) take windows twice as large; itwSliceWindow is this with NULL (every preset the plugin selects). */
int  itwSliceWindowFor(int dxgi_format, const void* settings, int width, int height, int64_t slice_pixels);

/* A whole mip chain, cube map or texture array in one call (IntelPlugin.cpp:229-255 makes one pad + CompressImageMT / DirectX::Compress call
 * per image of the ScratchImage).
 *
 * itwChainBytes: bytes the chain encodes to: the sum over images of ceil(w/4)*ceil(h/4)*GetBytesPerBlock(fmt) (== itwDdsLevelBytes per image).
 * -1 on bad arguments.  Host-only arithmetic, no device needed.
 *
 * itwCompressImageChain[Ex]: encodes `count` images (mip levels, cube faces, array items, in the caller's order) into `target`, one after
 * another, tightly packed: image i starts at the sum of the sizes of images < i -- for a DirectXTex ScratchImage (array item, face, mip:
 * DDS order) that is exactly imgCompressed[0].pixels and a DDS payload.  Same bytes as, for each image in order, the plugin's
 * DoPaddingToMultiplesOf4 + CompressImageMT (ISPC formats) or DirectX::Compress (BC4/BC5: partial blocks kept).
 *   * Formats: the twelve DXGI values above (71, 72, 77, 78, 80, 81, 83, 84, 95, 96, 98, 99) and ITW_FORMAT_ETC1_RGB8.  `settings` as in
 *     itwCompressImageSlicedEx: bc7_enc_settings* (BC7), bc6h_enc_settings* (BC6H), etc_enc_settings* (ETC1), ignored otherwise.
 *   * Pixels: RGBA8 (ETC1 ignores alpha), or RGBA16F for BC6H.
 *   * Images: any width and height >= 1, any `stride` >= the row's bytes.  Sizes that are not multiples of 4 are padded as the plugin pads
 *     them: edge replication for BC1, BC3, BC6H, BC7 and ETC1 (itwPadToMultipleOf4's rule), DirectXTex's partial-block fill for BC4 and BC5
 *     (CompressBlocksBC4/5's rule).
 *   * Pointers: all images host pointers, or all device pointers of the calling thread's current device; mixing them is an error.
 *     `target` may be either kind.  Synchronous either way, like itwCompressImageSliced.
 *   * One device: the calling thread's current device (a chain is not spread over several GPUs).
 *   * Progress: progress(i, count, user) is called for i = 1 .. count, in order, each call only once every image < i is in `target`.  A false
 *     return stops the job and the call returns false: images < i stay written, and so may images of work already in flight (as with the
 *     slice pipeline's windows).  `progress` runs on the calling thread while later work is in flight: it must not call back into this library.
 *   * Errors: count <= 0, a null pointer (images, target, an image's texels, null BC7 / BC6H / ETC1 settings), an ETC1 threshold < 1, a width or height < 1, a stride below
 *     the row's bytes, an unknown format, or mixed pointer kinds fail the call through the library's error mode before any device work
 *     starts; under ITW_ON_ERROR_RETURN it returns false and itwLastError() holds the message.
 *   * itwCompressImageChain with one of THIS library's CompressImage* trampolines resolves to the same path as the Ex call with the
 *     trampoline's preset; any other `cmpFunc` (for ETC1, which has no trampoline: every one) gets the plugin's literal loop: pad (host; device images on the device), then `cmpFunc`, per image.
 * How: consecutive images are gathered into groups of up to a slice-pipeline window of blocks (itwSliceWindowFor's ~131 072 / 262 144), each
 * group packed into one surface on the device and encoded as one; the groups run as the windows of itwCompressImageSliced do.  An image of
 * at least a window whose width and height are multiples of 4 is encoded in place as one whole-surface call. */
int64_t itwChainBytes(const rgba_surface* images, int count, int dxgi_format);
bool itwCompressImageChain(const rgba_surface* images, int count, uint8_t* target, CompressionFunc* cmpFunc,
                           int dxgi_format, ItwProgressFunc* progress, void* user);
bool itwCompressImageChainEx(const rgba_surface* images, int count, uint8_t* target, int dxgi_format,
                             const void* settings, ItwProgressFunc* progress, void* user);

/* Encode to an error budget: a cheap preset everywhere, an expensive one only where the cheap one misses.
 *
 * itwCompressImageRefined encodes `source` with `first_settings`, measures every block against its 16 source texels, and encodes with
 * `refine_settings` only the blocks whose error is above `max_block_sse` (the LISTED blocks); a listed block takes the second encoding
 * only where that is strictly better.  Blocks of a BCn stream depend on their own 16 texels alone, so EVERY block of `target` is, byte
 * for byte, the block CompressBlocksBC7 / BC6H emits for the whole surface under one of the two settings -- the reference's block.
 *   * Formats: BC7 (98, 99) with two bc7_enc_settings*, BC6H (95, 96) with two bc6h_enc_settings*.  Any other format is an error: only
 *     these two have more than one encoder.
 *   * Source: RGBA8, or RGBA16F for BC6H; width and height multiples of 4 and >= 4 (pad with itwPadToMultipleOf4[Device]); `stride` >= the
 *     row's bytes; at most ITW_MEASURE_MAX_BLOCKS (itw_decode.h) blocks.
 *   * Block error: what itwMeasureBlocks defines for block_sse -- squared code differences, integers, BC6H as 16-bit patterns -- summed
 *     over the channels in `channel_mask` only (bit 0 = R .. bit 3 = A, as itwStatsPsnr; 1..15).  With mask 15 the values are
 *     itwMeasureBlocks' own.  BC6H callers pass 7 (the decoders fill alpha with 0x3C00), and so do BC7 RGB presets on non-opaque sources.
 *   * Rule: A = the first tier's block, eA its error.  eA <= max_block_sse: A is written, tier_map 0.  Otherwise the block is listed;
 *     B = the refine tier's block, eB its error; eB < eA: B is written, tier_map 2; else A is written, tier_map 1 (ties keep the first
 *     tier).  The error of a block of the result is never above the first tier's.  max_block_sse = UINT64_MAX lists nothing and launches
 *     no second tier; 0 lists every block that is not exact.
 *   * Outputs: `target`, tightly packed blocks in raster order; `stats` (required, 8-byte aligned, stats_bytes = sizeof); `block_sse`
 *     (optional, one uint64 per block, 8-byte aligned): the error of the block written; `tier_map` (optional, one byte per block).
 *   * Pointers: each of source->ptr, target, stats, block_sse and tier_map may be a host pointer or a device pointer of the calling
 *     thread's current device.  One device; the calling thread's stream (itwSetStream).
 *   * SYNCHRONOUS for every pointer kind: the host reads one word -- the number of listed blocks -- back from the device between the two
 *     tiers.  For the same reason the call cannot be captured into a graph.
 *   * Errors: a null pointer (source, texels, target, either settings, stats), a format other than the four above, a width or height that
 *     is below 4 or no multiple of 4, a stride below the row's bytes, too many blocks, a mask of 0 or above 15, a stats_bytes other than
 *     sizeof(itw_refine_stats), a misaligned stats or block_sse: all fail through the library's error mode before any device work starts
 *     (under ITW_ON_ERROR_RETURN the call returns false and itwLastError() holds the message), and need no device.
 * Scratch memory (the list, the listed blocks' texels and second encodings, the maps the caller did not pass device memory for) belongs
 * to the calling thread and only grows; its worst case is the whole surface listed. */
typedef struct itw_refine_stats {
    uint64_t blocks;                   /* (width/4)*(height/4) */
    uint64_t listed;                   /* blocks whose first-tier error was > max_block_sse */
    uint64_t replaced;                 /* listed blocks whose second-tier encoding was STRICTLY better and was written */
    uint64_t sse_first, sse_final;     /* sum of the per-block errors: after the first tier / of the stream written */
    uint64_t worst_first, worst_final; /* largest per-block error: after the first tier / of the stream written */
} itw_refine_stats;                    /* may grow at its end; stats_bytes must be sizeof */

bool itwCompressImageRefined(const rgba_surface* source, uint8_t* target, int dxgi_format,
                             const void* first_settings, const void* refine_settings,
                             uint32_t channel_mask, uint64_t max_block_sse,
                             itw_refine_stats* stats, size_t stats_bytes,
                             uint64_t* block_sse, uint8_t* tier_map);

/* Encode to a number of refined blocks or to a summed error: the device picks the budget.
 *
 * itwCompressImageRefinedTo is itwCompressImageRefined for callers who know what they want to spend or reach rather than a per-block
 * budget, which nobody can know before the first tier has run.  The first tier's error map stays on the device; an exact select over it
 * gives the budget T, and the rest of a round is itwCompressImageRefined's: list the blocks above T, encode them with `refine_settings`,
 * keep a second encoding only where it is strictly better.  Formats, source, block error, channel mask, pointer kinds, alignment, scratch
 * and error mode are itwCompressImageRefined's; the call is synchronous and cannot be captured (the host reads the list length and one
 * more word per round).
 *   * select(k) over the CANDIDATES (the blocks still at tier 0): T = the (k+1)-th largest candidate error, counting equal values as
 *     often as they occur, or 0 when there are at most k candidates -- the smallest T among the candidate errors and 0 that leaves at
 *     most k candidates above it.  The round lists the candidates with error > T.  So k = 0 lists nothing, a group of equal errors that
 *     straddles rank k is left off the list as a whole (a round may list fewer than k blocks, never more), and T = 0 lists every candidate
 *     that is not exact.  Integers only: the same bits on every run.
 *   * Policy A, target_total_sse == UINT64_MAX: one round with k = max_listed.  `target`, `block_sse`, `tier_map` and `total` are byte
 *     for byte what itwCompressImageRefined(..., max_block_sse = T, ...) gives; rounds = 1, budget[0] = T, listed[0] = total.listed.
 *     (max_listed = UINT64_MAX: T = 0, every block that is not exact is listed.)
 *   * Policy B, a target: up to five rounds j = 0..4.  Before each round the call ends if the stream's summed block error is already
 *     <= target_total_sse, or if max_listed is used up.  Round j runs select(k_j), k_j = min(max_listed - blocks listed so far, q_j),
 *     q_j = max(1, blocks >> (4 - j)) for j < 4 and q_4 = blocks: a sixteenth, an eighth, a quarter, a half, then everything.  A block is
 *     refined at most once (tier_map 1 and 2 are no candidates), so the refine tier encodes at most `blocks` blocks in total; a round that
 *     lists nothing costs its select only and the next round follows.  Every block of the result is still the reference's block under one
 *     of the two settings and no block's error is above the first tier's.  An unreachable target runs all five rounds and reports
 *     target_met = 0.  itwPsnrToTotalSse turns a PSNR into a target.
 *   * Errors, on top of itwCompressImageRefined's: a null policy or stats, a policy_bytes / stats_bytes other than the sizeof, a misaligned
 *     stats; before any device work, no device needed. */
typedef struct itw_refine_policy {
    uint64_t max_listed;               /* most blocks the refine tier may encode over the whole call; UINT64_MAX = no cap */
    uint64_t target_total_sse;         /* stop once the stream's summed block error is <= this; UINT64_MAX = single round (policy A) */
} itw_refine_policy;
typedef struct itw_refine_target_stats {
    itw_refine_stats total;            /* as itwCompressImageRefined reports, over the whole call */
    uint32_t rounds;                   /* refine rounds that ran their select (0..5) */
    uint32_t target_met;               /* 1 if total.sse_final <= target_total_sse */
    uint64_t budget[5];                /* T of each round run, else 0 */
    uint64_t listed[5];                /* blocks listed per round */
} itw_refine_target_stats;             /* policy_bytes / stats_bytes must be the sizeof */

bool itwCompressImageRefinedTo(const rgba_surface* source, uint8_t* target, int dxgi_format,
                               const void* first_settings, const void* refine_settings, uint32_t channel_mask,
                               const itw_refine_policy* policy, size_t policy_bytes,
                               itw_refine_target_stats* stats, size_t stats_bytes,
                               uint64_t* block_sse, uint8_t* tier_map);

/* The inverse of itwStatsPsnr (itw_decode.h), host arithmetic in double: the largest summed error at which a width x height image,
 * measured over the channels of channel_mask, still has at least psnr_db: floor(peak^2 * n / 10^(psnr_db / 10)), n = width * height *
 * number of selected channels, peak as itwStatsPsnr.  The floor rounds the target DOWN, so a stream that meets it never reports less
 * than psnr_db.  UINT64_MAX (no target) where itwStatsPsnr has no answer: BC6H or an unknown format, a mask without one of the four
 * channels, a width or height < 1, a psnr_db that is NaN or infinite; BC6H callers pass a summed error. */
uint64_t itwPsnrToTotalSse(int dxgi_format, int width, int height, uint32_t channel_mask, double psnr_db);

/* A whole mip chain, cube map or texture array to an error budget, in one call.
 *
 * itwCompressImageChainRefined / itwCompressImageChainRefinedTo are itwCompressImageRefined / itwCompressImageRefinedTo over the blocks of
 * a whole chain as ONE population: level 0 and a 2 x 2 tail mip compete for the same budget, the same list and the same select.
 *   * Images: `images`, `count`, the layout of `target` and its size (itwChainBytes) are itwCompressImageChainEx's: any width and height
 *     >= 1, any stride >= the row's bytes, RGBA8 or RGBA16F for BC6H, all images host pointers or all device pointers.  Formats and the
 *     two settings structs as itwCompressImageRefined (95, 96, 98, 99).
 *   * Encoding: block j of the chain's concatenated block list is the block itwCompressImageChainEx writes for it under one of the two
 *     settings -- encoded from the edge-replicated image.  With max_block_sse = UINT64_MAX, `target` equals
 *     itwCompressImageChainEx(first_settings) byte for byte.
 *   * Block error: itwMeasureBlocks' block_sse for the block's image: squared code differences over the texels INSIDE the image only,
 *     summed over the channels of channel_mask.  Replicated padding never counts, under either tier (itwMeasureChain of `target` reports
 *     the same sums).  The rule (tiers 0 / 1 / 2, ties keep the first tier) and every field of itw_refine_stats are
 *     itwCompressImageRefined's, over all blocks of the chain.
 *   * Maps and stats: block_sse and tier_map hold one entry per block of the concatenated list, indexed as itwDecodeChain indexes `modes`.
 *     image_stats (optional; `count` entries, 8-byte aligned) holds the same seven fields over image i's blocks alone: blocks, listed,
 *     replaced, sse_first and sse_final sum to the totals, the maxima of worst_first / worst_final over i are the totals'.
 *   * itwCompressImageChainRefinedTo: the select, the quotas (`blocks` = the chain's block count), the rounds, budget[] and listed[] are
 *     itwCompressImageRefinedTo's, unchanged, over the chain.
 *   * itwChainPsnrToTotalSse: itwPsnrToTotalSse with n = the sum over images of width * height, times the selected channels; UINT64_MAX in
 *     the same cases, and for count < 1 or null `images`.
 *   * Pointers: target, stats, image_stats, block_sse and tier_map may each be a host or a device pointer.  Synchronous and not capturable,
 *     like the single-image calls; one device, the calling thread's stream.
 *   * Errors: everything itwCompressImageChainEx and itwCompressImageRefined[To] refuse, a summed block count above ITW_MEASURE_MAX_BLOCKS
 *     and a misaligned image_stats fail through the library's error mode before any device work starts, and need no device.
 * How: the whole chain is gathered once into one packed surface of min(1024, n) blocks per row (the copy is the price of one population);
 * the first tier encodes it into scratch and the first n blocks are copied to `target` at the end. */
bool itwCompressImageChainRefined(const rgba_surface* images, int count, uint8_t* target, int dxgi_format,
                                  const void* first_settings, const void* refine_settings,
                                  uint32_t channel_mask, uint64_t max_block_sse,
                                  itw_refine_stats* stats, size_t stats_bytes,
                                  itw_refine_stats* image_stats,
                                  uint64_t* block_sse, uint8_t* tier_map);
bool itwCompressImageChainRefinedTo(const rgba_surface* images, int count, uint8_t* target, int dxgi_format,
                                    const void* first_settings, const void* refine_settings, uint32_t channel_mask,
                                    const itw_refine_policy* policy, size_t policy_bytes,
                                    itw_refine_target_stats* stats, size_t stats_bytes,
                                    itw_refine_stats* image_stats,
                                    uint64_t* block_sse, uint8_t* tier_map);
uint64_t itwChainPsnrToTotalSse(const rgba_surface* images, int count, int dxgi_format, uint32_t channel_mask, double psnr_db);

/* Pad to multiples of 4 by edge replication (IntelPlugin.cpp:893-928): the step immediately before the ABI.
 * pixel_size = 4 (RGBA8) or 8 (RGBA16F).  Host version: returns a surface whose ptr was allocated with malloc()
 * (free with itwFreeSurface); the reference allocates with new[] and leaves ownership to the caller likewise.
 * Device version: `out_ptr` is a caller-allocated device buffer of ((w+3)&~3)*pixel_size x ((h+3)&~3) bytes, tight
 * pitch; asynchronous on the calling thread's stream (itwSetStream). */
rgba_surface itwPadToMultipleOf4(const rgba_surface* input, int pixel_size);
void itwFreeSurface(rgba_surface* s);
void itwPadToMultipleOf4Device(const rgba_surface* input, int pixel_size, uint8_t* out_ptr);

/* Photoshop's interleaved planes -> the encoder's surface, on the device (IntelPlugin.cpp:741-810 ConvertToBCFrom8/16/
 * 32Bit and :291-366 ConvertToBC6From8/16/32Bit): `src` holds width*height pixels of `planes` (1..4) interleaved
 * channels of `depth` bits (8, 16 = Photoshop's 0..32768 range, 32 = float); missing colour planes become 0, alpha is
 * opaque unless has_alpha (then plane 3; the reference's 32-bit -> half variant reads plane 2, kept).  `dst` is a
 * tightly pitched RGBA8 / RGBA16F surface.  Device pointers, asynchronous on the calling thread's stream.
 * gamma_correct applies the reference's pow(v, 1/2.2) to 32-bit input.  Returns 0, -1 on bad arguments. */
int itwConvertToRGBA8Device(const void* src, int depth, int planes, int has_alpha, int gamma_correct, int width, int height, uint8_t* dst);
int itwConvertToRGBA16FDevice(const void* src, int depth, int planes, int has_alpha, int width, int height, uint16_t* dst);

/* The normal-map stages of the save path (IntelPlugin.cpp:2103-2106 FlipXYChannelNormalMap :1506-1545, :2149-2152 NormalizeNormalMapChain
 * :1550-1613).  `ops` is a bit set; the flips apply first, then the normalise -- the reference's order.  Alpha is never touched, blue only
 * by the normalise.  Per texel, IEEE fp32 with every operation rounded on its own:
 *   RGBA8    flip: R = 255 - R and / or G = 255 - G.  normalise: r, g, b = (float)(code - 128); m = sqrtf((r*r + g*g) + b*b); m > 0: s = 127.0f / m and
 *            each channel becomes (uint8_t)(x*s + 128.0f) (truncation); otherwise the texel becomes (128, 128, 255).
 *   RGBA16F  flip: half(1.0f - float(h)).  normalise: m as above over the three halves widened to float; m > 0: s = 1.0f / m and each channel
 *            becomes half(x*s); otherwise (0, 0, 0x3C00).  half() rounds to nearest even, as itwConvertToRGBA16FDevice.  NaN and infinite
 *            inputs give what IEEE arithmetic gives; which NaN pattern comes out is not specified.
 *
 * itwPrepareNormalMapChain: in place over `count` images of any size >= 1 and any stride >= the row's bytes; pixel_size 4 (RGBA8) or 8
 * (RGBA16F).  All images host pointers or all device pointers.  Device pointers: one launch over the whole chain, asynchronous on the calling
 * thread's stream.  Host pointers: staged through the thread's buffer; returns synchronised.  Nothing outside width x height of an image is
 * written: row padding stays as it is.  Returns 0, also for count == 0 or ops == 0; -1, before any device work, for a null pointer,
 * count < 0, a pixel_size other than 4 or 8, unknown ops bits, a width or height < 1, a stride below the row's bytes, texels that are not
 * pixel_size aligned, or mixed host and device pointers.
 *
 * Height maps.  With ITW_NORMAL_FROM_HEIGHT in `ops` the images handed in are height maps (bump, displacement), and DirectXTex's
 * ComputeNormalMap (DirectXTexNormalMaps.cpp:22-244, Texconv's -nmap / -nmapamp) turns each into a tangent-space normal map before the bits
 * above apply with their usual meaning.  The further bits count only together with ITW_NORMAL_FROM_HEIGHT; without it every bit above 7 is
 * unknown, as it always was:
 *   ITW_HEIGHT_CHANNEL(c)    0 and 1 red, 2 green, 3 blue, 4 alpha, 5 luminance (r*0.2125f + g*0.7154f) + b*0.0721f; 6..15 are refused
 *   ITW_HEIGHT_MIRROR_U, _V  the neighbour beyond an edge is the edge's own column (row); without them the axis wraps to the opposite edge
 *   ITW_HEIGHT_INVERT_SIGN   the normal is negated (CNMAP_INVERT_SIGN)
 *   ITW_HEIGHT_OCCLUSION     alpha becomes the occlusion term (CNMAP_COMPUTE_OCCLUSION); without it alpha is 1
 *   ITW_HEIGHT_AMPLITUDE(h)  the amplitude, the bits of an IEEE half, finite and above 0 (0x0001 .. 0x7BFF; 1.0 is 0x3C00), widened to float
 * Bits 0x8, 0x10, 0x40, 0x80 and bit 31 are unknown.  Red channel, wrap, amplitude 1: 0x3C000120.
 * Per texel, IEEE fp32, every operation rounded on its own.  The height h of a texel is the chosen component as its kind loads it: an
 * RGBA8 code c is (float)c * (1.0f / 255.0f), an int8 code max((float)c * (1.0f / 127.0f), -1.0f), a half is widened, a float is taken as
 * it is.  With v0, v1, v2 the heights of rows y - 1, y, y + 1 and [0], [1], [2] the columns x - 1, x, x + 1 (a 1 x 1 image is its own eight
 * neighbours):
 *   dzx = ((((v0[0] - v0[2]) + (v1[0] - v1[2])) + (v2[0] - v2[2])) * amplitude) / 6.0f
 *   dzy = ((((v0[0] - v2[0]) + (v0[1] - v2[1])) + (v0[2] - v2[2])) * amplitude) / 6.0f
 *   c = cross((-1, 0, dzx), (0, -1, dzy)) as six products and three differences; m = sqrtf((c.x*c.x + c.y*c.y) + c.z*c.z); n = c / m, true
 *   divides; an infinite or NaN m gives NaN in all three.  Occlusion: delta sums the positive (neighbour - centre) differences, row by row;
 *   delta *= 0.125f * amplitude; delta > 0: r = sqrtf(1.0f + delta*delta), alpha = (r - delta) / r.
 * A biased RGBA8 target stores (+-0.5f * n) + 0.5f, a multiply then an add, each component as (uint8_t)(min(max(v, 0), 1) * 255.0f + 0.5f)
 * with NaN -> 0: a flat map is (128, 128, 255, 255).  RGBA16F and RGBA8_SNORM targets store n or -n: halves clamped to +-65504 and rounded to
 * nearest even with NaN -> 0x7E00, int8 codes by the signed sources' rule below.  One divergence from the reference: under MIRROR_V its row
 * above row 0 is a partial copy for sources narrower than RGBA32F (a memcpy of the source's row pitch over a row of float vectors); here
 * row -1 is row 0 for every kind.
 * Calls that take the bit: itwPrepareNormalMapChain (pixel_size 4: RGBA8 heights to a biased RGBA8 map; 8: RGBA16F to RGBA16F; in place
 * for the caller, the sources are first copied into the thread's buffer), itwQuantizeNormalMapChain (int8, half or float heights to
 * RGBA8_SNORM; a target that overlaps any source's bytes is refused), itwCompressImageMipped / itwCompressImageMippedEx (RGBA8 formats other
 * than 81 / 84: the stage writes level 0 of the device-side chain from the bases, then the call's own order follows) and
 * itwCompressSignedNormalMapMipped (the stage replaces the widening of level 0, heights differenced at the source's own precision).
 * itwCompressNormalMapChain, itwCompressSignedNormalMapChain, itwCompressNormalMapBC5 and itwCompressNormalMapBC5S refuse it: they see one
 * texel or one block at a time. */
enum { ITW_NORMAL_FLIP_X = 1, ITW_NORMAL_FLIP_Y = 2, ITW_NORMAL_NORMALIZE = 4, ITW_NORMAL_FROM_HEIGHT = 0x20,
       ITW_HEIGHT_MIRROR_U = 0x1000, ITW_HEIGHT_MIRROR_V = 0x2000, ITW_HEIGHT_INVERT_SIGN = 0x4000, ITW_HEIGHT_OCCLUSION = 0x8000 };
#define ITW_HEIGHT_CHANNEL(c)   ((uint32_t)(c) << 8)
#define ITW_HEIGHT_AMPLITUDE(h) ((uint32_t)(h) << 16)
int itwPrepareNormalMapChain(const rgba_surface* images, int count, int pixel_size, uint32_t ops);

/* itwCompressImageChainEx with the stages above applied to every texel as the chain's gather copies it: the same formats (the texel size
 * follows from the format: RGBA16F for BC6H, RGBA8 otherwise, the bytes of an RGBA8_SNORM source treated as codes like any other), images,
 * pointer kinds, progress contract, errors and return value.  The stream is byte for byte itwCompressImageChainEx over copies prepared with
 * itwPrepareNormalMapChain; the sources are never written.  With ops != 0 an image that itwCompressImageChainEx would encode in place goes
 * through the gather too (one copy more); ops == 0 is itwCompressImageChainEx.  Unknown ops bits fail through the error mode. */
bool itwCompressNormalMapChain(const rgba_surface* images, int count, uint8_t* target, int dxgi_format,
                               const void* settings, uint32_t ops, ItwProgressFunc* progress, void* user);

/* Signed normal sources: what a BC5_SNORM normal map is made from.  (The calls above speak the plugin's biased 8-bit convention only; they
 * keep it.)  A signed normal source is an image of 4-component texels of one of three kinds, named by the texel's size, `texel_bytes`:
 *   4   RGBA8_SNORM  int8 codes, each loaded as max((float)v * (1.0f / 127.0f), -1.0f): itw_bc45.h's rule
 *   8   RGBA16F      halfs, widened exactly
 *   16  RGBA32F      floats, as they are
 * The working value is the float vector (x, y, z, a).  `ops` takes ITW_NORMAL_FLIP_X / _FLIP_Y / _NORMALIZE with their SIGNED meaning, the
 * flips first, then the normalise; IEEE fp32, every operation rounded on its own, no contraction:
 *   flip       x = -x and / or y = -y (exact)
 *   normalise  m = sqrtf((x*x + y*y) + z*z); m > 0: s = 1.0f / m and x, y, z become x*s, y*s, z*s; otherwise (a NaN length included)
 *              (0, 0, 1).  Alpha is never touched.  The RGBA16F normalise above without its rounding to half.
 *   quantise   per component: NaN -> 0; otherwise c = min(max(v, -1.0f), 1.0f), p = c * 127.0f, code = (int8_t)rintf(p), round to nearest
 *              even.  DirectXMath is not in the reference tree: this line is the definition, as for the load rule.  -128 never comes out;
 *              with ops == 0 every int8 code maps to itself (-128 to -127), directly and through a half.
 *
 * itwQuantizeNormalMapChain: out of place, `count` sources of any size >= 1 and any stride >= the row's bytes into RGBA8_SNORM targets of
 * the same sizes, all four components quantised.  targets[i] may be sources[i] itself when texel_bytes == 4.  All pointers host or all
 * device.  Device pointers: one launch over the whole chain, asynchronous on the calling thread's stream.  Host pointers: staged through the
 * thread's buffer; returns synchronised.  Nothing outside width x height of a target is written.  Returns 0, also for count == 0; -1,
 * through the error mode and before any device work, for a null pointer, count < 0, a texel_bytes other than 4, 8 or 16, unknown ops bits,
 * a width or height < 1, a target whose size differs from its source's, a stride below the row's bytes, source texels that are not
 * texel_bytes aligned or target texels that are not 4-byte aligned, or mixed host and device pointers.  The fused encoder of such a source
 * is itwCompressNormalMapBC5S (itw_bc45.h). */
int itwQuantizeNormalMapChain(const rgba_surface* sources, int texel_bytes, const rgba_surface* targets, int count, uint32_t ops);

/* itwCompressImageChainEx for DXGI formats 81 (BC4_SNORM) and 84 (BC5_SNORM) over signed normal sources of `texel_bytes` 4, 8 or 16: the
 * chain's gather applies the definition above to every texel it copies, so the stream is byte for byte itwCompressImageChainEx over images
 * quantised by itwQuantizeNormalMapChain, and no image is encoded in place.  The chain call's images (rows at least width * texel_bytes
 * bytes apart), pointer kinds, progress contract, errors and return value; the sources are never written.  Any other format, a texel_bytes
 * other than 4, 8 or 16, and unknown ops bits fail through the error mode before any device work. */
bool itwCompressSignedNormalMapChain(const rgba_surface* images, int count, int texel_bytes, uint8_t* target, int dxgi_format, uint32_t ops,
                                     ItwProgressFunc* progress, void* user);

/* The signed normal-map save path from base images in one call (declared here, described with the mip chains below: it takes
 * itwCompressImageMipped's argument rules and launch limits).  A composition of the stages:
 *   1. the `items` bases, signed normal sources of `texel_bytes`, are widened into level 0 of a device-side RGBA16F chain: int8 becomes
 *      half(load rule), half is copied, float takes the mip filter's RGBA16F store rule (clamp to +-65504, round to nearest even, NaN ->
 *      0x7E00).  The flips of `ops` are folded into this widening: a negation is exact and commutes with both filters;
 *   2. itwGenerateMipChain over that chain, as it stands (RGBA16F is the texel format whose filters are pinned to the reference);
 *   3. itwCompressSignedNormalMapChain with texel_bytes 8 and only the NORMALIZE bit of `ops`: the normalise runs in fp32 on every level
 *      inside the gather, with no pass of its own and no rounding to half between the normalise and the quantisation.
 * dxgi_format 81 or 84; levels == 0: the full chain; the bases are not written.  Returns as itwCompressImageMipped does. */
bool itwCompressSignedNormalMapMipped(const rgba_surface* bases, int items, int levels, int texel_bytes, uint32_t ops, uint8_t* target,
                                      int dxgi_format, ItwProgressFunc* progress, void* user);

/* ConvertToCubeMapFromCross (IntelPlugin.cpp:1200-1265) as six VIEWS into `cross`, in the order +X -X +Y -Y +Z -Z: the faces of a horizontal
 * cross are width/4 x height/3 (truncating quotients) at cells (column, row) {2,1} {0,1} {1,0} {1,2} {1,1} {3,1}; when width < height the
 * cross is vertical, the faces are width/3 x height/4 and the last cell is {1,3}.  No rotation and no copy, as the reference's CopyRectangle
 * calls; the views share `cross`'s stride and feed itwCompressImageChainEx / itwCompressNormalMapChain directly (itw_decode.h documents the
 * inverse).  pixel_size 4, 8 or 16 (RGBA32F: a signed normal source).  Host arithmetic only.  Returns 0; -1 for a null pointer, a pixel_size other than 4, 8 or 16, or a cross smaller
 * than 4 x 3 (3 x 4 when vertical). */
int itwCubeCrossFaces(const rgba_surface* cross, int pixel_size, rgba_surface faces[6]);

/* Mip chains: GenerateMipMaps, the save path's fourth stage (IntelPlugin.cpp:2112-2146), on the device.
 *
 * Sizes.  Level l of a w x h base is max(1, w >> l) x max(1, h >> l); a full chain has 1 + floor(log2(max(w, h))) levels (_CountMips).
 * Level l is filtered from level l-1 AS STORED, that is after rounding to the texel format.
 * Filter.  The plugin passes TEX_FILTER_DEFAULT | TEX_FILTER_SEPARATE_ALPHA (plus TEX_FILTER_FORCE_NON_WIC for BC6H, :2117-2121); off
 * the WIC path DEFAULT means BOX when the base's width and height are both powers of two, else LINEAR (DirectXTexMipmaps.cpp:2615, :2803),
 * chosen once per chain from the base.  All four channels are filtered alike (the non-WIC filters have no premultiplied path, so
 * SEPARATE_ALPHA changes nothing).  IEEE fp32, every operation rounded on its own, no contraction:
 *   box     (_Generate2DMipsBoxFilter :715-805; AVERAGE4, Filters.h:33-39)  v = ((p0 + p1) + p2) + p3; v = v * 0.25f, with p0 = (row 2y,
 *           column 2x), p1 = (2y+1, 2x), p2 = (2y, 2x+1), p3 = (2y+1, 2x+1); when the source height is 1, row 2y+1 is row 2y; when the
 *           source width is 1, column 2x+1 is column 2x.
 *   linear  (_Generate2DMipsLinearFilter :809-917; _CreateLinearFilter and BILINEAR_INTERPOLATE, Filters.h:66-106)  per axis, clamped, no
 *           wrap: scale = float(source) / float(dest); srcB = (float(u) + 0.5f) * scale + 0.5f; isrcB = (ptrdiff_t)srcB; isrcA = isrcB - 1,
 *           clamped to 0; isrcB clamped to source - 1; weight0 = 1.0f + float(isrcB) - srcB with the clamped isrcB, in the order written;
 *           weight1 = 1.0f - weight0.  The texel is wy0 * (r0[u0]*wx0 + r0[u1]*wx1) + wy1 * (r1[u0]*wx0 + r1[u1]*wx1).
 *   RGBA16F -- the pinned case: the reference forces these functions for BC6H.  Load: the half widened exactly.  Store
 *           (DirectXTexConvert.cpp:1634-1646): clamp to [-65504, 65504], then float -> half by IEEE round to nearest even, the rule of
 *           itwConvertToRGBA16FDevice.  A NaN result (the reference's XMVectorClamp passes it through) stores the one pattern 0x7E00.
 *           +-Inf inputs make NaN under both filters (inf - inf, 0 * inf).
 *   RGBA8   -- THE LIBRARY'S OWN RULE, pinned to no byte of the reference: on Windows the reference sends 8-bit chains through WIC's closed
 *           Fant scaler, and DirectXMath's XMStoreUByteN4 is not part of its tree.  The same two filters on the raw codes as fp32 values
 *           0..255 (no division by 255), stored as (uint8_t)min(v + 0.5f, 255.0f); for the box that is exactly (a + b + c + d + 2) >> 2.
 *           The bytes of an RGBA8_SNORM surface are treated as codes like any other.
 *   RGBA8 with sRGB colour (ITW_MIP_SRGB) -- THE LIBRARY'S OWN RULE as well: the reference never passes TEX_FILTER_SRGB, and DirectXMath's
 *           XMColorSRGBToRGB is not part of its tree.  Without the flag an sRGB texture's codes are averaged as if they were light (a 0 / 255
 *           checkerboard gives 128 where linear light gives 188); the format code is never read as a request, the flag alone is.
 *           R, G, B are sRGB coded; A is linear and keeps the RGBA8 rule above exactly.  With f(x) = x / 12.92 for x <= 0.04045, else
 *           ((x + 0.055) / 1.055)^2.4 (IEC 61966-2-1):
 *             decode  D[c], c = 0..255, the fp32 nearest to f(c / 255);
 *             encode  E(v) = the number of k in 1..255 with v >= T[k], T[k] the fp32 nearest to f((k - 0.5) / 255): the nearest code in
 *                     the encoded domain; a value equal to a threshold goes up; values above 1 (the linear filter's weights can produce
 *                     them by an ulp) give 255; -0 and 0 give 0.
 *           The same two filters, unchanged in order and rounding, run on D[code] for R, G, B and the result is stored as E(v); level l is
 *           filtered from level l-1 as stored, as always.  T is strictly increasing and every constant image keeps its code at every
 *           level.  Both tables are csrc/srgb_tables.h, generated by tools/gen_srgb_tables.py with `decimal` at 60 digits;
 *           itwSrgbToLinear(c) is D[c] and itwLinearToSrgb(v) is E(v), on the host, over those tables.
 * Mip chains: cubic and triangle.  Two further filters of the same file, chosen by a flag bit and then run on EVERY level of every chain,
 * whatever the base's size (level l from level l-1 as stored, as always); with neither bit the chain is the default's above, byte for byte.
 * The same arithmetic rules: IEEE fp32, every operation rounded on its own, no contraction, on the host and in the kernels.  RGBA16F is
 * pinned byte for byte to the reference's own functions (tests/golden/mipfilter_ref.npz); the cited lines are the authority.
 *   cubic   (ITW_MIP_CUBIC; _Generate2DMipsCubicFilter :921-1103; _CreateCubicFilter, bounduvw, CUBIC_INTERPOLATE, Filters.h:123-205)  per
 *           axis: scale = float(source) / float(dest); srcB = (float(u) + 0.5f) * scale - 0.5f; iB = bound((ptrdiff_t)srcB) (in range as it
 *           is at every ratio >= 1); x = srcB - float(iB); the taps are bound(iB - 1), iB, bound(iB + 1), bound(iB + 2), where bound(t) with
 *           wrap turns t < 0 into t + source and t > source - 1 into t - source, and then, wrap or not, clamps into [0, source - 1].  The
 *           value over taps p0..p3: a0 = p1; d0 = p0 - a0; d2 = p2 - a0; d3 = p3 - a0; a1 = (d2 - third*d0) - sixth*d3; a2 = half*d0 + half*d2;
 *           a3 = (sixth*d3 - sixth*d0) - half*d2; res = ((a0 + a1*x) + a2*(x*x)) + a3*((x*x)*x), with the fp32 constants 1.f/3.f, 1.f/6.f and
 *           0.5f.  A texel is that expression in y over C0..C3, the four row results over the x taps of the four y-tap rows (:1076-1088).
 *           At the chain's 2:1 ratio x is 0.5 and the weights are (-1, 9, 9, -1) / 16 per axis: sharper than the box, with negative lobes.
 *   triangle (ITW_MIP_TRIANGLE; _Generate2DMipsTriangleFilter :1107-1313; TriangleFilter::_Create, Filters.h:249-418)  a tent prefilter
 *           that weights every source texel under the footprint.  Per axis _Create(source, dest, wrap) gives every source index an ordered
 *           list of (destination, weight), restated on the host as written: the two passes j = 0, 1 over src = float(u + j) - 0.5f, the
 *           clamp of destMin / destMax to [0, dest] without wrap, the fold of k < 0 and k >= dest with wrap, weight = (d0 + d1) * scaleInv
 *           - src (1 and 0 at the clamped ends), accumWeight += (d1 - d0) * (j ? 1 - weight : weight), the merging of consecutive equal
 *           destinations, and the drop of weights not above TF_EPSILON = 0.00001f.  An output texel starts at 0 and receives
 *           acc = texel * (yweight * xweight) + acc, a multiply then an add (XMVectorMultiplyAdd's SSE form), in the reference's order of
 *           arrival: source rows ascending; within a row, source columns ascending; within one source texel, its row entries outside and
 *           its column entries inside.  The device gathers: the host inverts the lists, order preserved, and the lists of all levels
 *           travel behind the chain's image table in the same single upload; nothing is read back.
 *   wrap    (ITW_MIP_WRAP_U along x, ITW_MIP_WRAP_V along y: TEX_FILTER_WRAP_U / _V)  for tiling textures, whose clamped border taps would
 *           otherwise grow a seam at every level.  Under the DEFAULT filter the bits are accepted and change nothing, and that is the
 *           reference's behaviour, not an omission: for source >= dest the linear filter's `isrcA < 0` and `isrcB >= source` branches
 *           (Filters.h:66-102) fire only for 1 -> 1, where the wrapped and the clamped answer coincide, and the box filter never looks past
 *           an edge.  TEX_FILTER_MIRROR_* changes no byte of a definition-sized chain: at ratios >= 1 a cubic tap is at most one texel
 *           outside, where bounduvw's mirror equals its clamp, and the triangle filter never reads the flag.  Its bits, ITW_MIP_MIRROR_U /
 *           _V, therefore belong to the free-size chain below, where an upscale's +2 tap lands two texels outside and the two differ.
 *   texel kinds  all three, with the loads and stores above: RGBA16F (0x7E00 for a NaN; +-Inf makes NaN under cubic, and under triangle
 *           where both signs meet in one sum); RGBA8 on raw codes; RGBA8 with ITW_MIP_SRGB, the filter on D[code] and the store E(v), which
 *           already sends anything below T[1] to 0 and anything above 1 to 255.  The cubic filter's negative lobes give the raw-code
 *           store its one missing case: (uint8_t)min(max(v, 0.0f) + 0.5f, 255.0f), the rule above for every v >= 0.
 *   launches  each level is its own launch (the pyramid route is the box filter's); ITW_MIP_PER_LEVEL is accepted and changes nothing.
 *   alpha options (itwGenerateMipChainAlpha, below)  coverage_ref combines with both filters: it is a pass over the finished chain.
 *           weight_colour = 1 with either filter bit is refused: a quotient of sums with negative weights is not an average, and the
 *           weighted triangle kind is left for later.
 *   refused, through the error mode, before any device work and with nothing written: ITW_MIP_CUBIC | ITW_MIP_TRIANGLE together, and the
 *           weight_colour combination.  Bits 2, 8, 0x100, 0x4000 and up stay unknown and refused; 0x200 .. 0x2000 are the free-size chain's.
 * Mip chains: free sizes (ITW_MIP_RESIZE; itwGenerateMipChain only).  DirectX::Resize's non-WIC filters (DirectXTexResize.cpp:
 * _ResizePointFilter :242, _ResizeBoxFilter :300, _ResizeLinearFilter :362, _ResizeCubicFilter :448, _ResizeTriangleFilter :608, chosen by
 * _PerformResizeUsingCustomFilters :784) are the mip functions over a free (source, dest) pair, plus a point filter.  With the bit the
 * size of every level is whatever its surface says: any width and height >= 1, larger or smaller than the level above, independently per
 * axis; level l has one size across the items.  Level 0 is read and never written; level l >= 1 is written, filtered from level l-1 as
 * stored.  levels == 2 is DirectX::Resize (texconv's -w / -h / -pow2); more levels make a chain of the caller's own sizes, for example
 * 4000 x 3000 -> 4096^2 -> 2048^2.  levels is 2 .. 32; levels <= 1 stays "nothing to do"; the full chain's length is no limit here.
 * Strides, alignment, pointer kinds, staging and stream behaviour are the call's as always.  Every level pair is its own launch
 * (ITW_MIP_PER_LEVEL is accepted and changes nothing).  RGBA16F is pinned byte for byte to the reference's own functions
 * (tests/golden/resize_ref.npz); RGBA8 and RGBA8 with ITW_MIP_SRGB run the same arithmetic between the loads and stores above.
 *   filter, per pair of levels  no filter bit: box when 2 * dw == sw and 2 * dh == sh, else linear.  Or one of:
 *   point   (ITW_MIP_POINT)  source column (x * ((sw << 16) / dw)) >> 16 in 64-bit integers (the reference's running sum is that product),
 *           rows alike.  The texel goes through the kind's own load and store: RGBA8 and sRGB codes are copied, and an RGBA16F texel
 *           follows the store rule above, +-Inf becomes +-65504 and a NaN 0x7E00.
 *   linear  (ITW_MIP_LINEAR)  _CreateLinearFilter as written (Filters.h:66-102) WITH its wrap branches: isrcA < 0 becomes source - 1 and
 *           isrcB >= source becomes 0 under wrap, and weight0 = 1.0f + float(isrcB) - srcB is formed from the folded isrcB.
 *           Refused: the linear filter, named or chosen by default, with a wrap bit on an axis where dest >= source and source > 1.  There
 *           the fold fires on the last texels and the weights it leaves are no interpolation (4 -> 8 ends in r[3] * -3.25 + r[0] * 4.25):
 *           an artefact of the reference that is neither pinned nor "fixed" here; the cubic and triangle filters wrap at any ratio.  On
 *           axes with dest < source the branches do not fire and the bits change nothing, as in a definition-sized chain.
 *   cubic, triangle  (ITW_MIP_CUBIC, ITW_MIP_TRIANGLE)  the arithmetic above at any ratio.  (ptrdiff_t)srcB truncates toward zero, so the
 *           first texels of an upscale have a small negative x: that is the reference's output.  A triangle destination that no list
 *           entry reaches is written as zeros, what an accumulator that is never added to holds.
 *   mirror  (ITW_MIP_MIRROR_U / _V: TEX_FILTER_MIRROR_U / _V)  bounduvw's mirror branch (Filters.h:136-146): t < 0 becomes -t - 1 and
 *           t > source - 1 becomes 2 * source - 1 - t, then the clamp.  Read by the cubic filter only; wrap wins where both are set.
 *           Accepted and without effect under point, box, linear ("mirror is the same case as clamp for linear") and triangle.
 *   refused, through the error mode, before any device work and with nothing written: two of POINT / LINEAR / CUBIC / TRIANGLE together;
 *           POINT, LINEAR or a MIRROR bit without ITW_MIP_RESIZE; the linear-wrap case above; levels > 32; a level below 1 x 1; items that
 *           disagree on a level's size; a written level of more than 262 140 rows or more than 65 535 items (one launch).
 *           itwGenerateMipChainAlpha and the itwCompressImageMipped* calls refuse all five bits as unknown.
 * Stated divergence.  The reference's box filter sets urow2 / urow3 once before its level loop (:740-741) and, once the height has reached 1,
 * re-points only urow1 (:746-749): from the level where the height is 1 while the width is still above 1, urow3 reads the second scanline
 * of an EARLIER level, which is no longer loaded (for a base of height 1: uninitialised storage).  Square and tall chains -- cube faces
 * among them -- are not affected.  The library takes the evident intent, row 2y+1 is row 2y: p1 = p0 and p3 = p2, ((a + a) + b) + b.
 *
 * itwMipLevels: the length of a full chain; 0 for a width or height below 1.
 * itwMipChainLayout: host arithmetic only.  Fills out[items * levels] in DDS order -- item-major, then level -- with tight rows, the images
 * packed one after another from `storage`, and returns the bytes needed.  levels == 0 means the full chain.  storage == NULL and out == NULL
 * is a size query (out alone: the pointers are the offsets).  -1 for a width or height below 1, items < 0, levels < 0 or above the full
 * chain, a pixel_size other than 4 or 8, or a row above 2^31 - 1 bytes.
 * itwGenerateMipChain: `images` is items * levels surfaces in that order; level 0 of each item holds the caller's texels and is never
 * written; levels 1 and up are written, width x height only.  Any stride at least the row's bytes, so levels may be views of a larger
 * canvas.  All pointers device or all host.  Device: asynchronous on the calling thread's stream.  Host: staged through the thread's
 * buffer -- only the bases go up, only the written levels come back -- and the call returns synchronised.  Power-of-two chains take the
 * pyramid route: a 64 x 64 tile of a level gives its part of the next six levels in one launch, a last launch takes a level of at most
 * 64 x 64 down to 1 x 1 (a 4096^2 chain: two launches); ITW_MIP_PER_LEVEL forces one launch per level, as every other chain takes, for
 * comparison and measurement.  Both routes write the same bytes.  ITW_MIP_SRGB (pixel_size 4 only) selects the sRGB colour kind above; it
 * combines with ITW_MIP_PER_LEVEL, takes the same routes and launches, and both routes write the same bytes.  ITW_MIP_CUBIC, ITW_MIP_TRIANGLE
 * and ITW_MIP_WRAP_U / _V: "Mip chains: cubic and triangle" above.  ITW_MIP_RESIZE and the bits that go with it: "Mip chains: free sizes"
 * above, whose size rules replace this paragraph's for such a call.  Flag value 2 is unassigned and
 * refused like any unknown bit.  Returns 0, also for items == 0 or levels <= 1 (nothing to do); -1,
 * through the library's error mode and before any device work, for a pixel_size other than 4 or 8, an unknown flag bit, ITW_MIP_SRGB with
 * pixel_size 8, items < 0, a
 * null pointer, a level whose size is not the definition's, items whose bases differ in size, levels above the full chain, a stride
 * below the row's bytes, texels that are not pixel_size aligned, mixed host and device pointers, or more than one launch covers (more
 * than 65 535 items, a base of more than 524 280 rows, more than 2^31 - 1 tiles of 64 x 64 over all items).
 * itwCompressImageMipped: the save path from base images in one call.  `bases` (items of them, one size, host or device) are copied into
 * level 0 of a device-side chain of `levels` levels (0: the full chain), then, IN THE REFERENCE'S ORDER: the flips of `normal_ops`
 * (ITW_NORMAL_FLIP_X / _Y) on level 0 only, as FlipXYChannelNormalMap runs before the mips; the chain is generated; ITW_NORMAL_NORMALIZE on
 * every level, as NormalizeNormalMapChain runs after them; the chain is encoded into `target` exactly as itwCompressImageChainEx encodes
 * it (items * levels images in DDS order; itwChainBytes / itwDdsFileBytes give the size).  The bases are never written.  Formats, texel
 * kinds, settings, progress contract (1 .. items * levels), pointer kinds of `target`, errors and return value are the chain call's; on
 * top of them unknown ops bits, bases of different sizes, levels < 0 or above the full chain, misaligned texels, mixed pointer kinds
 * and itwGenerateMipChain's launch limits fail through the error mode before any device work.  From host bases only the bases go up and only blocks come down.
 * itwCompressImageMippedEx: the same with `mip_flags` (ITW_MIP_*) handed to the chain's generation; itwCompressImageMipped is this call with
 * mip_flags == 0, byte for byte.  With ITW_MIP_SRGB the colour of every level is filtered in linear light, whatever `dxgi_format` says --
 * 72 / 78 / 99 without the flag keep the plain rule's bytes.  ITW_MIP_CUBIC / ITW_MIP_TRIANGLE and ITW_MIP_WRAP_U / _V choose the chain's
 * filter and addressing for every format and go with normal_ops.  Unknown flag bits, both filter bits together, and ITW_MIP_SRGB with an RGBA16F format (95 / 96), a signed
 * format (81 / 84) or normal_ops != 0 (a normal map is not colour), fail through the error mode before any device work.
 * itwSrgbToLinear, itwLinearToSrgb: D[code] and E(v) of the sRGB colour kind; host arithmetic only. */
enum { ITW_MIP_PER_LEVEL = 1, ITW_MIP_SRGB = 4,
       ITW_MIP_CUBIC = 0x10, ITW_MIP_TRIANGLE = 0x20, ITW_MIP_WRAP_U = 0x40, ITW_MIP_WRAP_V = 0x80 };
/* the free-size chain's bits ("Mip chains: free sizes"): itwGenerateMipChain alone takes them */
enum { ITW_MIP_RESIZE = 0x200, ITW_MIP_POINT = 0x400, ITW_MIP_LINEAR = 0x800, ITW_MIP_MIRROR_U = 0x1000, ITW_MIP_MIRROR_V = 0x2000 };
int itwMipLevels(int width, int height);
int64_t itwMipChainLayout(int width, int height, int items, int levels, int pixel_size, uint8_t* storage, rgba_surface* out);
int itwGenerateMipChain(const rgba_surface* images, int items, int levels, int pixel_size, uint32_t flags);
bool itwCompressImageMipped(const rgba_surface* bases, int items, int levels, uint32_t normal_ops, uint8_t* target, int dxgi_format,
                            const void* settings, ItwProgressFunc* progress, void* user);
bool itwCompressImageMippedEx(const rgba_surface* bases, int items, int levels, uint32_t normal_ops, uint32_t mip_flags, uint8_t* target,
                              int dxgi_format, const void* settings, ItwProgressFunc* progress, void* user);
float itwSrgbToLinear(uint8_t code);
uint8_t itwLinearToSrgb(float v);

/* Mip chains of cut-out textures (RGBA8 with an alpha test: foliage, fences, hair, decals): two more of THE LIBRARY'S OWN RULES, pinned to
 * no byte of the reference (it passes TEX_FILTER_DEFAULT | TEX_FILTER_SEPARATE_ALPHA and has neither).  Both are options of itw_mip_alpha,
 * both default to off, and with both off not one byte differs from itwGenerateMipChain's.  RGBA8 only; levels, sizes and the choice of
 * filter are those of "Mip chains" above: box when the base's width and height are powers of two, else linear, level l from level l-1 as
 * stored, the base never written.
 *
 * A. Alpha-weighted colour (weight_colour = 1).  A texel of alpha 0 carries whatever colour the painter left there, and the plain filter
 *    averages it into its visible neighbours: dark or white fringes from level 1 on.  Per output texel:
 *      each source tap is widened as always: raw codes, or D[code] for R, G, B under ITW_MIP_SRGB;
 *      R, G, B of each tap are multiplied by that tap's alpha code, p = c * a, one fp32 multiply;
 *      the same filter expression, in the same order and rounding, runs over the premultiplied colour and over alpha: P[k] and va, the
 *      filtered, unrounded alpha;
 *      if va > 0 the colour is P[k] / va, one correctly rounded fp32 division; otherwise it is what the plain rule gives for that texel;
 *      alpha is stored from va exactly as always, colour by the kind's own store: (uint8_t)min(v + 0.5f, 255.0f), or E(v) under ITW_MIP_SRGB.
 *    For the box on raw codes that is (2 * sum(a_i * c_i) + sum(a_i)) / (2 * sum(a_i)) in integers, round-half-up.
 * B. Coverage kept per level (coverage_ref = r, 1 .. 255; 0: off).  Averaging alpha and then testing it is not averaging the test: the
 *    share of texels that pass `alpha >= r` drifts from level to level and a thin object dissolves with distance.  The chain is first
 *    generated whole with coverage off (weighting and sRGB as asked); then, per item, the alpha of every level >= 1 is replaced.  All
 *    arithmetic is in 64-bit integers:
 *      level 0 has N0 texels, cov0 of them with a >= r;
 *      a level of n texels has the target K = (cov0 * n + N0 / 2) / N0, floor;
 *      ge[t] is the number of its texels with a >= t;
 *      t* is the t in 1 .. 255 that minimises the triple (|ge[t] - K|, |t - r|, t), compared lexicographically;
 *      every texel's alpha becomes a' = min(255, (a * r) / t*), floor.
 *    So #(a' >= r) == ge[t*] exactly, t* == r leaves the level's bytes as they were, alpha 0 stays 0, and R, G, B are never touched.  Every
 *    count is an integer sum: the same bits on every run.  A base of more than 2^31 texels is refused with coverage on.
 *
 * itwGenerateMipChainAlpha: itwGenerateMipChain with pixel_size 4 and the two rules.  `flags` takes ITW_MIP_PER_LEVEL and ITW_MIP_SRGB with
 * the same meaning, routes and pointer rules, and the filter and wrap bits of "Mip chains: cubic and triangle" (coverage_ref goes with
 * either filter, weight_colour = 1 with neither); alpha == NULL is both options off.  `report` (host memory, items * levels rows in DDS order, or
 * NULL) receives per image its texels, the count with a >= r before (covered_plain) and after (covered) the rescale, and t* (threshold);
 * level 0 rows hold covered_plain = covered = cov0 and threshold = r.  With `report` the call ends with a synchronise of the thread's
 * stream; without it the call is as asynchronous as itwGenerateMipChain is for the same pointers.  Coverage adds three launches -- the
 * histograms of every level, the thresholds, the rescale -- and one table upload, whatever the number of items and levels, and nothing on
 * the host is read between them.  items == 0 or levels <= 1: nothing to do, nothing reported.  Returns 0; -1, through the error mode,
 * before any device work and with nothing written, for struct_size != 16, reserved != 0, weight_colour > 1, coverage_ref > 255, a report
 * without coverage_ref, and everything itwGenerateMipChain refuses for pixel_size 4.
 * itwCompressImageMippedAlpha: itwCompressImageMippedEx with normal_ops 0 and the rules handed to the chain's generation; with both off it
 * writes that call's payload.  The encode is the same itwCompressImageChainEx.  Refused as ITW_MIP_SRGB is, for the same reason -- the
 * texels are not RGBA8 colour: DXGI formats 95 / 96 and 81 / 84.
 * itwAlphaCoverage: per RGBA8 image, the number of texels with alpha >= alpha_ref (0 .. 255) into covered[count] (host memory): the count
 * the coverage rule uses, so a caller can check a chain or choose r.  Images of any sizes >= 1, any stride at least the row's bytes, all
 * host or all device pointers; returns synchronised.  0, or -1 through the error mode. */
typedef struct itw_mip_alpha    { uint32_t struct_size /* 16 */, weight_colour /* 0|1 */, coverage_ref /* 0..255 */, reserved /* 0 */; } itw_mip_alpha;
typedef struct itw_mip_coverage { uint64_t texels, covered_plain, covered; uint32_t threshold, reserved; } itw_mip_coverage;   /* 32 bytes, one per image, DDS order */
int itwGenerateMipChainAlpha(const rgba_surface* images, int items, int levels, uint32_t flags, const itw_mip_alpha* alpha, itw_mip_coverage* report);
bool itwCompressImageMippedAlpha(const rgba_surface* bases, int items, int levels, uint32_t mip_flags, const itw_mip_alpha* alpha, uint8_t* target,
                                 int dxgi_format, const void* settings, ItwProgressFunc* progress, void* user);
int itwAlphaCoverage(const rgba_surface* images, int count, int alpha_ref, uint64_t* covered);

/* Mip chains: volumes.  GenerateMipMaps3D (DirectXTexMipmaps.cpp:2884-2983) and its five _Generate3DMips*Filter functions (:1371-2497) on
 * the device: 3D LUTs, fog and cloud density, 3D noise.  Level l of a w x h x d base is max(1, w >> l) x max(1, h >> l) x max(1, d >> l); a
 * full chain has 1 + floor(log2(max(w, h, d))) levels.  A chain is a list of SLICES (rgba_surface images) in DDS volume order, LEVEL-MAJOR:
 * the d slices of level 0, then the max(1, d >> 1) slices of level 1, and so on.  That order is a
 * volume .dds file's payload (itw_dds.h, ITW_DDS_VOLUME), and the list is what itwCompressImageChainEx, itwDecodeChain and itwMeasureChain
 * take as it is.  Level l is filtered from level l-1 AS STORED.  IEEE fp32, every operation rounded on its own, no contraction; the per-axis
 * arithmetic, the three texel kinds and their loads and stores are those of "Mip chains" and "Mip chains: cubic and triangle" above.
 * RGBA16F is pinned byte for byte to the reference's own functions (tests/golden/mip3d_ref.npz); RGBA8 and RGBA8 with ITW_MIP_SRGB run the
 * same fp32 arithmetic between the library's loads and stores.  Once the depth has reached 1 every filter takes the reference's 2D branch
 * of the same function, which is the 2D chain's expression for that filter over the one slice.
 *   no filter bit  GenerateMipMaps3D's default (:2921-2926): BOX when width, height and depth are all powers of two, TRIANGLE otherwise.
 *           THIS DIFFERS FROM THE 2D CALL, whose default for other sizes is linear.
 *   box     (_Generate3DMipsBoxFilter :1517-1685; only reachable by the default)  AVERAGE8 in its written order (Filters.h:41-51): the taps
 *           (2x, 2y), (2x, 2y+1), (2x+1, 2y), (2x+1, 2y+1) of slice 2z, then the same four of slice 2z+1, summed left to right, times
 *           0.125f.  Once the depth is 1, AVERAGE4 as the 2D chain.  An axis of size 1 gives the second tap = the first.
 *   point   (ITW_MIP_POINT; :1371-1513)  source index (u * ((source << 16) / dest)) >> 16 per axis in 64-bit integers; the texel goes
 *           through the kind's own load and store (RGBA16F: +-Inf becomes +-65504, a NaN 0x7E00).
 *   linear  (ITW_MIP_LINEAR; :1689-1878)  _CreateLinearFilter on three axes and TRILINEAR_INTERPOLATE's written association
 *           (Filters.h:108-112): z.w0 * (y.w0 * (a*x.w0 + b*x.w1) + y.w1 * (c*x.w0 + d*x.w1)) over slice z.u0, plus z.w1 * the same over
 *           slice z.u1.  Here the two bits select the filter WITHOUT ITW_MIP_RESIZE.
 *   cubic   (ITW_MIP_CUBIC; :1882-2258)  _CreateCubicFilter per axis; CUBIC_INTERPOLATE along x for the four y-tap rows of each of the four
 *           z-tap slices, then along y per slice, then along z over the four slice values, in the written order.
 *   triangle (ITW_MIP_TRIANGLE; :2261-2497)  TriangleFilter::_Create per axis.  A destination texel starts at 0 and receives
 *           acc = texel * ((zweight * yweight) * xweight) + acc, a multiply then an add, over source slices ascending, then rows, then
 *           texels; within one source texel its z entries outside, its y entries next, its x entries inside.  The device gathers over the
 *           three inverted lists, which gives the same order.  A depth of 1 has the one z weight 1.0f, so a depth-1 volume writes the 2D
 *           triangle chain's bytes.
 *   wrap    (ITW_MIP_WRAP_U / _V / _W: TEX_FILTER_WRAP_U / _V / _W)  read by the cubic and triangle filters' table builders.  Box, point and
 *           linear accept the bits and write the same bytes: at ratios >= 2 they never reach past an edge.  ITW_MIP_WRAP_W is read beside
 *           ITW_MIP_VOLUME only; without that bit every call keeps refusing 0x100 as unknown.
 *   launches  one per level for every filter: lanes along x, grid (x tiles, y tiles, destination slices).  ITW_MIP_PER_LEVEL is accepted and
 *           changes nothing.
 * Stated divergence, the one.  The reference's box filter keeps urow3 / vrow3 pointing into the old urow1 / vrow1 once the height has
 * reached 1 while the width has not (:1552-1564): it reads a stale scanline, the defect stated for the 2D box above.  The library takes its
 * 2D rule in every axis: an axis of size 1 gives the second tap = the first.
 *
 * No new entry point: a volume goes through the calls above with ITW_MIP_VOLUME (0x8000) in their flags, which changes what two
 * arguments mean and nothing else about the calls.  Without the bit every call is what it was, and ITW_MIP_VOLUME and ITW_MIP_WRAP_W stay
 * unknown bits to itwGenerateMipChainAlpha and itwCompressImageMippedAlpha (alpha weighting and coverage are not offered for volumes).
 * Host arithmetic a caller does itself: a full chain has itwMipLevels(max(width, height), depth) levels; the first `levels` levels have
 * the sum over l < levels of max(1, depth >> l) slices; a packed chain is those slices one after another, each
 * max(1, w >> l) x max(1, h >> l) texels with tight rows (itwChainBytes over such a list gives the encoded size).
 * itwGenerateMipChain(slices, depth, levels, pixel_size, flags | ITW_MIP_VOLUME): `images` is the slice list in that order and `items` the
 * DEPTH of level 0; the `depth` slices of level 0 hold the caller's texels and are never written; levels 1 and up are written, width x
 * height only.  Any stride at least the row's bytes, so slices may be views of a larger canvas.  All pointers device or all host.  Device:
 * asynchronous on the calling thread's stream.  Host: staged through the thread's buffer -- only level 0 goes up, only the written levels
 * come back -- and the call returns synchronised.  pixel_size 4 (RGBA8; with ITW_MIP_SRGB the sRGB colour kind) or 8 (RGBA16F).  Returns
 * 0, also for depth == 0 or levels <= 1 (nothing to do); -1, through the library's error mode, before any device work and with nothing
 * written, for a pixel_size other than 4 or 8; two filter bits together; ITW_MIP_RESIZE or a mirror bit (DirectXTex has no 3D resize); an
 * unknown flag bit; ITW_MIP_SRGB with pixel_size 8; depth < 0; a null pointer; a slice whose size is not the definition's; levels above the
 * full chain; a stride below the row's bytes; texels that are not pixel_size aligned; mixed host and device pointers; or more than one
 * launch covers: a base of more than 131 071 slices (level 1 is a grid plane per slice, 65 535) or of more than 524 280 rows.
 * itwCompressImageMippedEx(base_slices, depth, levels, 0, mip_flags | ITW_MIP_VOLUME, target, ...): the volume save path in one call.
 * `bases` are the `items` = depth base slices (one size, host or device); they are copied into level 0 of a device-side chain of `levels`
 * levels (0: the full chain), the chain is generated as above under `mip_flags`, and the slice list is encoded into `target` exactly as
 * itwCompressImageChainEx encodes it: a volume .dds file's payload (itw_dds.h).  The bases are never written.  Formats, texel kinds,
 * settings, padding rules, progress contract (1 .. slices), pointer kinds of `target`, errors and return value are the chain call's; on
 * top of them everything the generation refuses, normal_ops != 0, and ITW_MIP_SRGB with an RGBA16F (95 / 96) or signed (81 / 84) format,
 * fail before any device work.  itwCompressImageMipped (no flags word), the Alpha call and itwCompressSignedNormalMapMipped take no volume. */
enum { ITW_MIP_WRAP_W = 0x100,       /* TEX_FILTER_WRAP_W; read only beside ITW_MIP_VOLUME, unknown and refused without it */
       ITW_MIP_VOLUME = 0x8000 };    /* itwGenerateMipChain, itwCompressImageMippedEx: the image list is a volume's slices, `items` its depth */

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
