/*
 * itw_decode.h -- BC1 / BC3 / BC4 / BC5 (UNORM and SNORM) / BC7 / BC6H(unsigned) block decoding on the GPU: the step immediately after the ABI in
 * the reference's preview and load paths, where DirectXTex's Decompress() (D3DXDecodeBC1/BC3/BC7/BC6HU,
 * 3rdParty/DirectXTex/DirectXTex/BC.cpp, BC6HBC7.cpp:1077-1210, 1937-2140) turns the blocks back into texels
 * (IntelPlugin.cpp:1059, 2558).  Written from the format definitions; used here for preview-style round trips and
 * for whole-surface validity / PSNR checks of the encoder's output without leaving HBM.
 */
#ifndef ITW_DECODE_H
#define ITW_DECODE_H

#include <stddef.h>
#include <stdint.h>
#include "ispc_texcomp.h"   /* rgba_surface */

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)   /* the library is built with -fvisibility=hidden: only what the headers declare is exported */

/* Decodes (width/4)*(height/4) tightly packed blocks in raster block order into a surface of `out_stride` bytes per
 * texel row: RGBA8 for BC1 / BC3 / BC7, (R,0,0,255) / (R,G,0,255) RGBA8 for BC4 / BC5 (the layout D3DXDecodeBC4U/BC5U
 * produce, BC4BC5.cpp:373-385, 449-462; 8-bit values by the format's integer definition, rounded to nearest),
 * RGBA16F bit patterns for BC6H (alpha = 1.0 = 0x3C00).  width and height are multiples of 4 (a BC4/BC5 stream of a
 * partial surface decodes to the padded size).
 * BC4_SNORM / BC5_SNORM decode to RGBA8_SNORM, int8 codes (R,0,0,127) / (R,G,0,127): the layout D3DXDecodeBC4S/BC5S produce
 * (BC4BC5.cpp:388-400, 465-478) with R = rint(127 * its float).  As integers, with s0, s1 the endpoint bytes and -128 read as -127:
 * levels 0, 1 = s0, s1; if the RAW bytes have r0 > r1, level 1+i = round(((7-i)*s0 + i*s1) / 7), i = 1..6; else level 1+i =
 * round(((5-i)*s0 + i*s1) / 5), i = 1..4, and levels 6, 7 = -127, 127 (round to nearest; no ties with odd divisors).  Never -128.
 * dxgi_format: one of the ITW_DXGI_FORMAT_BC* values of itw_dispatch.h (71,72,77,78,80,81,83,84,95,96,98,99), or ITW_FORMAT_ETC1_RGB8 (0x8D64):
 * ETC1, 8-byte blocks, RGBA8 texels with alpha filled with 255, whole blocks only; modes 0 = individual, 1 = differential, -1 = a differential
 * block whose base + delta leaves 0..31 (invalid in ETC1; decoded with the sum modulo 32 and counted in reserved_blocks).
 * ITW_FORMAT_BC1A_UNORM / _SRGB (0x83F1 / 0x8C4D, BC1 with 1-bit alpha): synonyms of 71 / 72 in every entry point of this header -- the stream
 * is a BC1 stream, decoded, measured (itw_error_stats.dxgi_format says 71 / 72) and previewed by the same code.
 * ITW_FORMAT_BC3_DXTEX / _SRGB (0x83F3 / 0x8C4F, BC3 by DirectXTex's encoder): synonyms of 77 / 78 in every entry point of this header -- the
 * stream is a BC3 stream, decoded, measured (itw_error_stats.dxgi_format says 77 / 78) and previewed by the same code.
 * ITW_FORMAT_BC2_UNORM / _SRGB (0x83F2 / 0x8C4E, BC2 / DXT3): taken by every entry point of this header under these two codes (DXGI's 74 / 75
 * are refused like any unknown code; itw_dispatch.h says why): 16-byte blocks, RGBA8 texels, any size >= 1 in itwDecodeBlocks too (a
 * DirectXTex format, like the BC4 / BC5 group); the colour is always the four-colour palette whatever the order of the endpoints -- BC2 has
 * no 3-colour mode --, alpha is the texel's 4-bit code times 17, which is D3DXDecodeBC2's n / 15 exactly; no modes (0);
 * itw_error_stats.dxgi_format repeats the code given; own channels RGBA.
 * ITW_FORMAT_BC6H_SIGNED (0x8E8E, itw_dispatch.h): the SIGNED reading of a BC6H stream -- what a GPU shows for a texture labelled BC6H_SF16,
 * whoever wrote the file -- taken by itwDecodeBlocks (whole blocks), itwDecodeChain / itwDecodeImage (any size >= 1), itwMeasureBlocks,
 * itwMeasureChain and itwPreviewBlocks; 16-byte blocks, RGBA16F bit patterns, alpha 0x3C00, modes 0..13 and -1 as for 95.  Byte for byte
 * DirectXTex's D3DXDecodeBC6HS (BC6HBC7.cpp:1077-1235), the halves INTColor::ToF16(.., true) produces:
 *  1. endpoint 0.A is sign-extended at the base precision, every other endpoint at its own field width (the delta width in the transformed
 *     modes, the base width otherwise), in transformed and untransformed modes alike (:1143-1159);
 *  2. transformed modes: each other endpoint becomes (itself + 0.A) & ((1 << base) - 1), sign-extended again at the base precision (:582-594);
 *  3. Unquantize (:1316-1335): base >= 16 keeps the value; otherwise on the magnitude m: 0 -> 0, m >= (1 << (base - 1)) - 1 -> 0x7FFF, else
 *     ((m << 15) + 0x4000) >> (base - 1), and the sign is put back;
 *  4. a texel is (a * (64 - w) + b * w + 32) >> 6 on signed ints, an arithmetic shift;
 *  5. FinishUnquantize (:1351-1354): x < 0 ? -(((-x) * 31) >> 5) : (x * 31) >> 5;
 *  6. INT2F16 (BC.h:407-420): 0x8000 | magnitude for a negative value, no clamp, and zero is never -0.
 *  In the 16-bit mode (13) an endpoint can be -32768, and a texel that interpolates to exactly -32768 is (32768 * 31) >> 5 = 0x7C00 under the
 *  sign bit: 0xFC00, -Inf (the reference's recorded output has such texels).  +Inf and NaN patterns cannot occur: the largest positive
 *  result is 0x7BFF.  A reserved prefix gives 0, 0, 0, 0x3C00 and mode -1.  This library's ENCODER under code 96 still writes the reference's
 *  unsigned-coded blocks, as the reference does; a signed encoder does not exist here (itw_dispatch.h).
 * `blocks`, `out`, `modes` are host or device pointers, in any mix.  With all of them on the device the call is one kernel launch,
 * asynchronous on the calling thread's stream (itwSetStream): it allocates nothing, touches no buffer of the thread and can be captured
 * into a graph.  With any host pointer it stages through the calling thread's grow-only device buffer (the one itwDecodeChain uses;
 * no hipMalloc / hipFree per call) and returns synchronised.  A device `blocks` pointer is at least 4-byte aligned, `out` 4-byte (8 for
 * RGBA16F); rows that are 16-byte aligned are stored as vectors.
 * `modes` (optional, may be NULL): one int32 per block -- BC7: mode 0..7, -1 for the reserved all-zero-prefix block;
 * BC6H: mode 0..13 in kernel.ispc's numbering, -1 for a reserved prefix; BC1/BC3: 0.
 * Width and height must be multiples of 4, except for BC4 / BC5 (UNORM and SNORM), whose streams may end in partial blocks (cropped on
 * store; any size >= 1).  out_stride: a multiple of 4, at least the row's bytes, at most INT32_MAX.
 * This is a chain of one image through the kernel of itwDecodeChain below, under its own, older argument rules: it reads BC6H_SF16 (96)
 * as unsigned, and its size limit is not ITW_MEASURE_MAX_BLOCKS but what one launch covers, 2^31 - 1 blocks.
 * Returns 0; -1 before any device work for an unsupported format, a size or stride outside the rules above or more blocks than one launch
 * covers; -1 after a device failure, which is reported through the library's error mode (itw_amd.h: abort by default; in return mode the
 * message is kept for itwLastError). */
int itwDecodeBlocks(int dxgi_format, const uint8_t* blocks, int width, int height, uint8_t* out, int64_t out_stride, int32_t* modes);

/* ---- a whole mip chain / cube map / array, any size, in one call -------------------------------------------------------------------
 * The mirror image of itwCompressImageChain (itw_dispatch.h), and the load path's Decompress over every image of a file
 * (IntelPlugin.cpp:2461-2561).  `blocks`: the packed stream of `count` images as itwCompressImageChain lays it out (image i starts at the
 * summed sizes of the images before it, itwChainBytes; ceil(w/4)*ceil(h/4) blocks per image -- a DDS payload, itw_dds.h: itwDdsImage).
 * outs[i]: where image i's texels go -- ptr, width, height (any >= 1), stride (bytes, a multiple of 4, at least the row); RGBA8, int8
 * RGBA8_SNORM for BC4S / BC5S, RGBA16F bit patterns for BC6H_UF16 and ITW_FORMAT_BC6H_SIGNED.  ptr is 4-byte aligned (8 for RGBA16F).  Texels outside
 * width x height are never written: edge blocks are cropped on store, for every format.
 * dxgi_format: 71, 72, 77, 78, 80, 81, 83, 84, 95, 98, 99, 0x8D64 (ETC1), the BC1A / BC2 codes, ITW_FORMAT_BC6H_SIGNED.  BC6H_SF16 (96) itself
 * stays refused -- at itwDecodeBlocks the code reads as unsigned, and nothing here may pass for that --: a loader that finds 96 in a file's
 * header passes ITW_FORMAT_BC6H_SIGNED, and the file is then read as a GPU reads it.
 * modes (optional, may be NULL): one int32 per block of the concatenated block list, numbered as itwDecodeBlocks numbers them.
 * min_alpha (optional, may be NULL): one uint32 per image, the smallest decoded alpha code among the texels actually stored -- the load
 * path's IsAlphaAllOpaque question (255 = opaque) without a second pass.  For the formats that fill alpha it is that constant: BC4 / BC5
 * 255, BC4S / BC5S 127, BC6H 0x3C00.
 * One launch decodes every image.  The outs[i].ptr are all host or all device pointers; `blocks`, `modes`, `min_alpha` may each be either
 * (a device `blocks` pointer is at least 4-byte aligned).  With everything on the device the call is asynchronous on the calling thread's
 * stream (itwSetStream) and allocates nothing from a thread's second call on (the descriptor table is copied into a buffer the thread
 * keeps, so capturing a call of more than one image into a graph is not supported; a chain of one has no table).  With any host pointer it stages through the thread's grow-only buffer --
 * one upload of the stream, one launch, one strided download per image -- and returns synchronised.
 * Output surfaces may be views into one larger allocation.  Six cube faces of size s decoded straight into a 4s x 3s canvas at the cells
 * {2,1},{0,1},{1,0},{1,2},{1,1},{3,1} (column, row; the reference's crossedCoords, IntelPlugin.cpp:1435) ARE its
 * ConvertToHorizontalCrossFromCubeMap (:1421-1500), with no copy; mips to layers is the same with other offsets.
 * Returns 0 (also for count == 0); -1 before any device work for an unknown or refused format, count < 0, a null blocks / outs / ptr,
 * a width or height < 1, a stride below the row's bytes or not a multiple of 4, mixed host and device outputs, or more than
 * ITW_MEASURE_MAX_BLOCKS blocks in one image; -1 after a device failure (reported through the library's error mode, itw_amd.h). */
int itwDecodeChain(int dxgi_format, const uint8_t* blocks, const rgba_surface* outs, int count, int32_t* modes, uint32_t* min_alpha);
/* a chain of one */
int itwDecodeImage(int dxgi_format, const uint8_t* blocks, const rgba_surface* out, int32_t* modes, uint32_t* min_alpha);

/* ---- a viewport of an image, decoded where it is looked at -----------------------------------------------------------------------------
 * What the reference's preview dialog asks of IntelPlugin::FetchPreviewRGB (IntelPlugin.cpp:487-739) on every zoom, pan, channel toggle
 * or exposure change: a width x height RGB8 viewport of an image, nearest sampled.  Only the blocks the viewport looks at are decoded.
 * With W x H the image and (xt, yt) a viewport pixel, every step integer or IEEE arithmetic:
 *  1. fx = (double)(xt + x_offset) * zoom, one double multiply.  The pixel is outside when fx <= -1.0 or fx >= W; otherwise x = (int)fx,
 *     truncated toward zero, so -1 < fx < 0 shows column 0 and not the matte: what the reference's int(...) followed by `x < 0` does
 *     (:632-639).  The comparison comes first: a product beyond the int range is outside.  y likewise with H.  The bound is W, H and not
 *     the padded size: padding texels of edge blocks are never shown.
 *  2. Outside, the three bytes are matte_color & 0xFF, (matte_color >> 8) & 0xFF, (matte_color >> 16) & 0xFF.
 *  3. Channels (:585-624 with four planes).  m = options & ITW_PREVIEW_CHANNEL_MASK, and m == 0 reads as RED | GREEN | BLUE.  m exactly one
 *     of RED / GREEN / BLUE / ALPHA: all three bytes show that channel, and for ALPHA alone the exposure is taken as 1.  Any other m: byte 0
 *     shows R if RED is set, byte 1 G if GREEN is set, byte 2 B if BLUE is set -- and if ALPHA is set byte 2 shows A instead, whether or not
 *     BLUE is set: the reference's `channelIndex[2] = 3` (:610-611), kept as its behaviour.  A byte with no channel is 0.
 *  4. Value.  RGBA8 texels: the code itself, no exposure (:732-734).  RGBA16F texels (BC6H, and texel_bytes 8): v = (float)half * exposure as
 *     one fp32 multiply, d = (double)v, then d > 1 -> 255, d < 0 -> 0, NaN -> 0 (what the reference's cast gives on x86), otherwise
 *     (uint8_t)(d * 255.0), the product in double, truncated (FloatToByte, IntelPlugin.h:41-48; :676-678).  For BC6H this is also the
 *     reference's 32-bit-document route (:628-654, ConvertTo8Bit(x, false)), since DirectXTex widens the same halves.
 *     A decoded texel is exactly what itwDecodeImage stores, filled channels included: BC4 (R,0,0,255), BC6H alpha 0x3C00, ETC1 alpha 255.
 *     ITW_FORMAT_BC6H_SIGNED: the same step on the halves of the signed reading; a negative value, -Inf included, shows 0 because d < 0.
 *     This is the library's extension of the float route: the reference never previews a signed stream. */
#define ITW_PREVIEW_CHANNEL_RED   0x04   /* the reference's PREVIEW_OPTIONS values, IntelPlugin.h:248-261 */
#define ITW_PREVIEW_CHANNEL_GREEN 0x08
#define ITW_PREVIEW_CHANNEL_BLUE  0x10
#define ITW_PREVIEW_CHANNEL_ALPHA 0x20
#define ITW_PREVIEW_CHANNEL_MASK  0x3C

typedef struct itw_preview_view {
    int32_t  width, height;        /* viewport, pixels: 1 .. 16384 each */
    int32_t  x_offset, y_offset;   /* the reference's xo, yo: |value| <= 2^30 */
    double   zoom;                 /* source texels per viewport pixel (the reference passes 1.f / previewZoom, and divides by
                                      1 << mipLevel when it shows a mip: that division is the caller's); finite, > 0 */
    uint32_t options;              /* channel bits; bits outside ITW_PREVIEW_CHANNEL_MASK are ignored; no channel bit = RGB */
    uint32_t matte_color;          /* 0x00BBGGRR */
    float    exposure;             /* half-float sources only */
    uint32_t _pad;
} itw_preview_view;

/* Which of the kernel's two routes a call takes, from view->zoom alone.  zoom <= this: a workgroup owns a 64 x 16 tile of viewport pixels,
 * decodes each block under the tile once into LDS and samples from there (magnified views and views near 1:1, where a texel is shown
 * several times or neighbours share a block).  Above it: every lane decodes the block of its own pixel and keeps one texel.  At zoom 2 a
 * tile's footprint is at most 33 x 9 blocks, which is what the workgroup's LDS holds. */
#define ITW_PREVIEW_TILE_MAX_ZOOM 2.0

/* itwPreviewBlocks: the compressed pane.  `blocks`: the ceil(width/4) * ceil(height/4) blocks, raster order, of ONE image of any size >= 1
 * (an image of a chain; of a DDS / KTX payload via itwDdsImage / itwKtxImage).  dxgi_format: 71, 72, 77, 78, 80, 83, 95, 98, 99 or
 * ITW_FORMAT_ETC1_RGB8, the BC1A / BC2 codes or ITW_FORMAT_BC6H_SIGNED; BC4S / BC5S (81, 84) and BC6H_SF16 (96) are refused (the reference
 * previews neither; a BC6H_SF16 file is previewed under ITW_FORMAT_BC6H_SIGNED).
 * itwPreviewSurface: the original pane, through the same sampling code with a plain load in place of the decode.  source: RGBA8
 * (texel_bytes 4) or RGBA16F bit patterns (texel_bytes 8), any size >= 1, stride >= the row's bytes; a device source has ptr and stride
 * aligned to the texel (a host source: any).
 * out_rgb: height rows of width RGB8 pixels, out_stride >= 3 * width bytes apart, at any byte address; exactly 3 * width bytes of each row
 * are written and nothing else (dword stores where a row's address allows, bytes at a row's ends and for unaligned rows).
 * `view` is read at call time and travels as kernel arguments.  `blocks` / source->ptr and out_rgb are host or device pointers in any mix
 * (a device `blocks` is at least 4-byte aligned).  Everything on the device: one launch, asynchronous on the calling thread's stream
 * (itwSetStream); the call allocates nothing, touches no buffer of the thread and can be captured into a graph.  A host out_rgb is staged
 * through the thread's decode buffer (the one itwDecodeChain uses) and 3 * width bytes per row are copied back; of a host `blocks` only
 * the block rows the viewport can reach are uploaded (y is monotone in yt: one contiguous range of the stream), of a host source only those
 * texel rows, and nothing when the viewport misses the image.  Calls with a host pointer return synchronised.
 * Returns 0; -1 before any device work for an unknown or refused format, a null pointer, view_bytes != sizeof(itw_preview_view), a viewport
 * size or offset outside the ranges above, a zoom that is not finite and positive, an image size < 1 or more than ITW_MEASURE_MAX_BLOCKS
 * blocks, out_stride < 3 * width, a texel_bytes other than 4 or 8, or a source stride below its row; -1 after a device failure (reported
 * through the library's error mode, itw_amd.h). */
int itwPreviewBlocks(int dxgi_format, const uint8_t* blocks, int width, int height,
                     const itw_preview_view* view, size_t view_bytes, uint8_t* out_rgb, int64_t out_stride);
int itwPreviewSurface(const rgba_surface* source, int texel_bytes, const itw_preview_view* view, size_t view_bytes, uint8_t* out_rgb,
                      int64_t out_stride);

/* ---- measuring an encoded stream against its source ------------------------------------------------------------------------------
 * What a caller would compute by decoding the stream (the decoders above, at the padded size) and comparing the texels of `source`
 * with the decoded ones, code by code, as integers -- done in one kernel that decodes into registers, so the decoded surface never
 * exists in memory.  A "code" is the 8-bit channel value for the LDR formats and the 16-bit half-float bit pattern, read as an
 * unsigned integer, for BC6H (the space BC6H interpolates in).  All four channels are always reported, the values the decoders fill
 * in included (BC4 / BC5: 0 / 0 / 255, BC6H: alpha 0x3C00, BC1: its decoded alpha); the caller picks the channels that mean something.
 * BC4_SNORM / BC5_SNORM: `source` is RGBA8_SNORM and a code is the int8 value, a source code of -128 read as -127 (both mean -1.0);
 * the filled-in channels are 0 / 0 / 127, and max_abs is at most 254.
 * ITW_FORMAT_BC6H_SIGNED: a code is the integer the signed reading interpolates in: for half bits h, (h & 0x8000) ? -(h & 0x7FFF) :
 * (h & 0x7FFF) -- F16ToINT's signed map (BC.h:387-398) without its clamp; +0 and -0 are both 0.  Source and decoded texel go through the
 * same map, alpha included.  max_abs is at most 0xFFFE, so the largest block sum stays below 2^39 and ITW_MEASURE_MAX_BLOCKS holds;
 * itw_error_stats.dxgi_format repeats 0x8E8E and itwStatsPsnr is NaN, as for 95.
 * Every field is an integer: the same stream and source give the same bits on every run. */
typedef struct itw_error_stats {
    int32_t  dxgi_format, width, height;  /* what was measured: texels per row / rows actually compared */
    uint32_t reserved_blocks;             /* blocks whose mode is -1 (reserved prefix); they decode as itwDecodeBlocks decodes them */
    uint64_t blocks;                      /* ceil(width/4) * ceil(height/4) */
    uint64_t sse[4];                      /* per channel R,G,B,A: sum over compared texels of (source code - decoded code)^2 */
    uint32_t max_abs[4];                  /* per channel: largest |source code - decoded code| */
    uint64_t worst_block_sse;             /* largest per-block sum of the four channels' squared differences */
    uint32_t worst_block;                 /* raster index of the FIRST block that reaches it */
    uint32_t _pad;
    uint64_t mode_hist[16];               /* blocks per mode: BC7 0..7, BC6H 0..13, ETC1 0..1 (itwDecodeBlocks' numbering), others all in [0] */
} itw_error_stats;

/* The most blocks one image may have: the worst block is found with one 64-bit atomic maximum over (block sse, inverted index), and
 * BC6H's largest block sum, 64 * 0xFFFF^2 < 2^39, leaves 25 bits for the index.  A 16384 x 16384 surface has 2^24 blocks. */
#define ITW_MEASURE_MAX_BLOCKS 33554432

/* itwMeasureBlocks: `blocks` holds ceil(w/4)*ceil(h/4) tightly packed blocks in raster order for the w x h texels of `source` (any
 * w, h >= 1, for every format: what itwCompressImageChain emits for such an image); texels of edge blocks that lie outside the
 * source are padding and are not compared.  source: RGBA8, or RGBA16F bit patterns for BC6H; stride: any value >= the row's bytes.
 * block_sse (optional, may be NULL): one uint64 per block in raster order, that block's sum over the four channels; worst_block_sse
 * is the maximum of exactly these values, worst_block the first index that has it.
 * stats_bytes must be sizeof(itw_error_stats) (the struct may grow at its end).
 * `blocks`, source->ptr, `stats`, `block_sse` may each be a host or a device pointer; stats and block_sse are 8-byte aligned.  With any
 * host pointer the call stages and returns synchronised.  With all of them on the device it is asynchronous on the calling thread's
 * stream (itwSetStream), allocates nothing, writes every field of *stats on the device in stream order, and can be captured into a graph.
 * Returns 0; -1 before any device work for an unknown format, a null pointer, width or height < 1, a stride below the row's bytes,
 * a wrong stats_bytes, a misaligned stats / block_sse or more than ITW_MEASURE_MAX_BLOCKS blocks; -1 after a device failure (reported
 * through the library's error mode, itw_amd.h). */
int itwMeasureBlocks(int dxgi_format, const uint8_t* blocks, const rgba_surface* source, itw_error_stats* stats, size_t stats_bytes,
                     uint64_t* block_sse);

/* itwMeasureChain: `images` and the packed `blocks` as itwCompressImageChain lays them out (itw_dispatch.h): image i's blocks start
 * at the summed sizes of the images before it (itwChainBytes); stats[i] describes image i.  The images are all host or all device
 * pointers; `blocks` and `stats` may each be either.  Per-image launches on one stream; all-device calls are asynchronous. */
int itwMeasureChain(const rgba_surface* images, int count, const uint8_t* blocks, int dxgi_format, itw_error_stats* stats, size_t stats_bytes);

/* itwStatsPsnr: host arithmetic in double: 10*log10(255^2 * n / sum of sse[c]) over the channels c in channel_mask (bit 0 = R ..
 * bit 3 = A), n = width * height * number of selected channels.  +inf when the sum is 0; NaN for a BC6H stats (a code-space PSNR of
 * half floats is not a quantity this library defines) and for an empty mask.  For BC4_SNORM / BC5_SNORM stats the peak is 254, the width
 * of the int8 code range -127..127, in place of 255. */
double itwStatsPsnr(const itw_error_stats* stats, uint32_t channel_mask);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
