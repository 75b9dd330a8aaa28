/*
 * itw_bc45.h -- BC4 / BC5 block encoding on the GPU, UNORM and SNORM.
 *
 * The two formats the plugin offers that bypass ispc_texcomp: IntelPlugin.cpp:120-141 converts the document to an
 * RGBA8 scratch image (BC4: the red plane in every colour channel, BC5: red and green) and IntelPlugin.cpp:271-273
 * calls DirectXTex
 *     Compress(images, nimages, metadata, DXGI_FORMAT_BC4_UNORM | DXGI_FORMAT_BC5_UNORM, TEX_COMPRESS_DEFAULT, 0.5f, out)
 * (3rdParty/DirectXTex/DirectXTex/DirectXTexCompress.cpp:607, :73-186), which encodes each 4x4 block with
 * D3DXEncodeBC4U / D3DXEncodeBC5U (3rdParty/DirectXTex/DirectXTex/BC4BC5.cpp:403, :481).  The entry points below replace
 * that per-image call with the calling convention of the library's other encoders, so the trampolines of
 * itw_dispatch.h and a patched plugin can treat all six formats alike.
 *
 * src     RGBA8 surface (ispc_texcomp.h rgba_surface), R in the lowest byte.  BC4 encodes R; BC5 encodes R then G.
 *         Any width, height >= 1: like DirectXTex (and unlike the ISPC formats) partial blocks are kept, their missing
 *         columns / rows filled from source column / row {0,0,0,1}[i] (DirectXTexCompress.cpp:140-168).
 * dst     ceil(width/4) * ceil(height/4) blocks in raster order, 8 bytes (BC4) or 16 bytes (BC5: R block, G block),
 *         tightly packed (DirectXTex's pitch rule, DirectXTexUtil.cpp:601-619).
 * Host or device pointers, threading, streams and error behaviour: exactly as CompressBlocksBC1 (ispc_texcomp.h).
 *
 * The signed pair, CompressBlocksBC4S / CompressBlocksBC5S (DXGI_FORMAT_BC4_SNORM = 81 / BC5_SNORM = 84; what a tangent-space normal
 * map is stored in: the centre is exact and the range symmetric), is D3DXEncodeBC4S / D3DXEncodeBC5S (BC4BC5.cpp:424, :515) under the
 * same contract.  src is an RGBA8_SNORM surface: byte 0 (BC5S: bytes 0 and 1) of a texel is a two's-complement int8 code v, and the
 * value the encoder sees is
 *     t = max((float)v * (1.0f / 127.0f), -1.0f)          with 1.0f / 127.0f an fp32 constant
 * which is DirectXMath's SSE XMLoadByteN4 (the conversion DirectX::Compress applies to an R8G8B8A8_SNORM image); DirectXMath is not
 * part of the reference tree, so this line is the definition.  Codes -128 and -127 both are -1.0f, 127 is exactly 1.0f.  Endpoints
 * are never stored as -128 (FloatToSNorm, BC4BC5.cpp:161-182).
 */
#ifndef ITW_BC45_H
#define ITW_BC45_H

#include "ispc_texcomp.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)   /* the library is built with -fvisibility=hidden: only what the headers declare is exported */

void CompressBlocksBC4(const rgba_surface* src, uint8_t* dst);
void CompressBlocksBC5(const rgba_surface* src, uint8_t* dst);

/* The first BC4 / BC5 call on a device builds a 1 MiB index table there (csrc/bc4_bc5.hip): that one call allocates device memory and is not
 * stream-capturable; itwWarmupBC45() does the same ahead of time (see itw_amd.h for the asynchronous contract of device-pointer calls). */
void itwWarmupBC45(void);

void CompressBlocksBC4S(const rgba_surface* src, uint8_t* dst);
void CompressBlocksBC5S(const rgba_surface* src, uint8_t* dst);

/* The signed encoders have an index table of their own, built by the first signed call on a device or by itwWarmupBC45S(), under the
 * same rules; itwWarmupBC45() and the UNORM pair neither build nor need it. */
void itwWarmupBC45S(void);

/* A normal map to BC5 as the plugin saves it -- the only format its NORMAL MAP texture type takes (IntelPlugin.cpp:58 IsCombinationValid) --
 * in one kernel: FlipXYChannelNormalMap and NormalizeNormalMapChain (IntelPlugin.cpp:2103-2106, 2149-2152) are applied to the texels as the
 * BC5 encoder loads them.  `ops`: ITW_NORMAL_FLIP_X | ITW_NORMAL_FLIP_Y | ITW_NORMAL_NORMALIZE (itw_dispatch.h, which defines the per-texel
 * arithmetic).  The stream is byte for byte CompressBlocksBC5 of a copy prepared with itwPrepareNormalMapChain; `src` is not modified;
 * ops == 0 is CompressBlocksBC5.  CompressBlocksBC5's contract otherwise: any size >= 1, partial blocks kept, host or device pointers,
 * device pointers asynchronous on the calling thread's stream.  Unknown `ops` bits fail through the library's error mode before any device
 * work.  The first normalising call on a device uploads a 192 KiB scale table next to the index table, under that table's rules
 * (itwWarmupBC45() builds both). */
void itwCompressNormalMapBC5(const rgba_surface* src, uint8_t* dst, uint32_t ops);

/* A signed normal source to BC5_SNORM in one kernel.  `src` holds texels of `texel_bytes` 4 (RGBA8_SNORM), 8 (RGBA16F) or 16 (RGBA32F); the
 * per-texel definition of itw_dispatch.h ("signed normal sources": load, the flips and the normalise of `ops` in fp32, quantise to int8 with
 * round to nearest even) runs in the BC5S encoder's load.  The stream is byte for byte CompressBlocksBC5S of the RGBA8_SNORM image that
 * itwQuantizeNormalMapChain makes of `src`; `src` is not modified; texel_bytes 4 with ops 0 is CompressBlocksBC5S.  CompressBlocksBC5S's
 * contract otherwise: any size >= 1, partial blocks kept, host or device pointers, device calls asynchronous on the calling thread's stream
 * and capturable once itwWarmupBC45S() has run.  Device texels are 4-byte aligned (pointer and stride).  A texel_bytes other than 4, 8 or
 * 16 and unknown `ops` bits fail through the library's error mode before any device work. */
void itwCompressNormalMapBC5S(const rgba_surface* src, int texel_bytes, uint8_t* dst, uint32_t ops);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
