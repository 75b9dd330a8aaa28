/*
 * itw_dds.h -- DDS container for the encoder's block streams: the header DirectXTex's _EncodeDDSHeader writes for
 * the formats the plugin saves (3rdParty/DirectXTex/DirectXTex/DDS.h:38-236, DirectXTexDDS.cpp:441-675, data
 * order :1611-1700, pitch rule DirectXTexUtil.cpp:601-619), restated portably.  BC1_UNORM / BC3_UNORM use the legacy
 * 'DXT1' / 'DXT5' FourCC header (128 bytes incl. magic), BC4 / BC5 'BC4U' / 'BC5U' (UNORM; 'ATI1' / 'ATI2' are read as these) and
 * 'BC4S' / 'BC5S' (SNORM; DDS.h:83-93, DirectXTexDDS.cpp:64-70, 480-483); the _SRGB variants, BC7 and BC6H carry the 'DX10' extension
 * (148 bytes).  Mip chains: top level first; cube maps: 6 faces, each with its full chain.
 * BC2: a descriptor names it by the library's two codes, ITW_FORMAT_BC2_UNORM = 0x83F2 / ITW_FORMAT_BC2_UNORM_SRGB = 0x8C4E (itw_dispatch.h), as
 * every entry point does; 74 / 75 as descriptor codes are refused like any code the library does not read.  The FILE holds DXGI's own: 0x83F2
 * without an array is written with the legacy 'DXT3' FourCC (DirectXTexDDS.cpp:478), otherwise a 'DX10' header with 74; 0x8C4E always 'DX10'
 * with 75.  Read: 'DXT3' and 'DX10' 74 give 0x83F2, 'DX10' 75 gives 0x8C4E; the premultiplied spellings 'DXT2' and 'DXT4' read as BC2 and BC3
 * (77), which is DirectXTex's mapping (DirectXTexDDS.cpp:58-62) -- that the file's alpha is premultiplied is NOT reported: the descriptor has
 * no field for it.  16 bytes per block.
 * BC3 by DirectXTex's encoder: ITW_FORMAT_BC3_DXTEX = 0x83F3 / ITW_FORMAT_BC3_DXTEX_SRGB = 0x8C4F as descriptor codes write the header of
 * 77 / 78 ('DXT5', or 'DX10' for an array and for 0x8C4F); a header read back says 77 / 78, as the BC1A codes read back as 71 / 72.
 *
 * Below the DDS functions: the KTX 1.1 container for ETC1 streams (itwKtx*), which DDS cannot carry.
 */
#ifndef ITW_DDS_H
#define ITW_DDS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)   /* the library is built with -fvisibility=hidden: only what the headers declare is exported */

typedef struct ItwDdsDesc {
    uint32_t width, height;     /* top mip, texels */
    uint32_t mip_levels;        /* >= 1 */
    uint32_t dxgi_format;       /* DXGI_FORMAT_BCn_* value (71,72,77,78,80,81,83,84,95,96,98,99), or one of the BC1A / BC2 / BC3_DXTEX codes of itw_dispatch.h */
    uint32_t is_cubemap;        /* 0 / 1: six faces; ITW_DDS_VOLUME: a volume texture (below) */
    uint32_t array_size;        /* number of textures (cubes when is_cubemap); >= 1.  The DEPTH of a volume */
} ItwDdsDesc;

/* Volume textures (3D LUTs, fog and cloud density, 3D noise): is_cubemap = ITW_DDS_VOLUME and array_size = the depth of level 0, through the
 * same seven functions.  The header is what _EncodeDDSHeader writes for TEX_DIMENSION_TEXTURE3D (DirectXTexDDS.cpp:585-597):
 * dwFlags |= DDS_HEADER_FLAGS_VOLUME (0x00800000), dwCaps2 |= DDS_FLAGS_VOLUME (0x00200000), dwDepth = depth; the legacy FourCC where the
 * format has one (the 2D rule and format-code mapping, the BC1A / BC2 / BC3_DXTEX codes included), otherwise 'DX10' with
 * resourceDimension 4, arraySize 1 and miscFlag 0.  Payload (:1167-1200): LEVEL-MAJOR, the max(1, depth >> l) slices of level l one after
 * another, each max(1, w >> l) x max(1, h >> l), without gaps -- the packed stream of the chain calls over the slice list of
 * itwGenerateMipChain with ITW_MIP_VOLUME (itw_dispatch.h).  itwDdsImage's index and itwDdsWriteFile's `levels` run over the slices in that
 * order: index i is slice i - (slices of the levels before) of the level it falls in.  A volume is never an array or a cube. */
enum { ITW_DDS_VOLUME = 2 };

/* bytes of one mip level: max(1,(w+3)/4) * max(1,(h+3)/4) * bytes-per-block */
size_t itwDdsLevelBytes(uint32_t dxgi_format, uint32_t width, uint32_t height);
/* header bytes (incl. the 4-byte magic): 128 or 148; 0 if the format is not one of the BCn formats above */
size_t itwDdsHeaderBytes(const ItwDdsDesc* desc);
/* header + all faces / levels */
size_t itwDdsFileBytes(const ItwDdsDesc* desc);
/* Writes the header into dst (capacity >= itwDdsHeaderBytes); returns bytes written, 0 on error. */
size_t itwDdsWriteHeader(const ItwDdsDesc* desc, uint8_t* dst, size_t capacity);
/* Parses a header; returns its size (offset of the first block), 0 if not a BCn DDS this library writes.  A header with
 * DDS_HEADER_FLAGS_VOLUME (0x00800000 in dwFlags) is a volume, by DirectXTex's own test (DirectXTexDDS.cpp:323-328): it reads as
 * is_cubemap = ITW_DDS_VOLUME with the depth in array_size.  Earlier versions never looked at the flag and read a legacy-header volume
 * as a 2D texture, whose every level after the first then came from the wrong bytes; a caller that handles 2D files only checks
 * is_cubemap.  Refused: a volume flag with a DX10 dimension other than 3D (or the reverse), a DX10 volume with arraySize > 1, a depth of 0. */
size_t itwDdsReadHeader(const uint8_t* src, size_t size, ItwDdsDesc* desc);
/* Whole file: `levels[i]` points at the blocks of image i in file order (array item major, then face, then mip).
 * Returns bytes written (== itwDdsFileBytes) or 0. */
size_t itwDdsWriteFile(const ItwDdsDesc* desc, const uint8_t* const* levels, size_t nlevels, uint8_t* dst, size_t capacity);
/* Image `index` in file order (array item, face, mip): its size in texels and the offset of its blocks from the start of the file.
 * Returns the image's byte size, 0 when index is out of range or desc is not a format this library reads.  width, height and offset may
 * each be NULL.  The images follow each other without gaps, so image 0's offset to the end of the last image is the packed stream
 * itwDecodeChain (itw_decode.h) takes; host arithmetic only. */
size_t itwDdsImage(const ItwDdsDesc* desc, uint32_t index, uint32_t* width, uint32_t* height, size_t* offset);

/* ---- KTX 1.1 -------------------------------------------------------------------------------------------------------------------------
 * KTX 1.1 container for the encoder's ETC1 block streams (Khronos KTX File Format Specification 1.1), the one format DDS has no
 * code for.  It lives in this header because the set of product headers is fixed (tests/test_abi_boundary.py).  KTX carries the GL enum this library already uses as ETC1's
 * format code (ITW_FORMAT_ETC1_RGB8 = GL_ETC1_RGB8_OES = 0x8D64, itw_dispatch.h) in glInternalFormat.
 *
 * File: a 64-byte header -- the 12-byte identifier AB 4B 54 58 20 31 31 BB 0D 0A 1A 0A, then 13 little-endian uint32:
 * endianness 0x04030201, glType 0, glTypeSize 1, glFormat 0, glInternalFormat 0x8D64, glBaseInternalFormat 0x1907 (GL_RGB),
 * pixelWidth, pixelHeight, pixelDepth 0, numberOfArrayElements 0, numberOfFaces 1 or 6, numberOfMipmapLevels >= 1,
 * bytesOfKeyValueData -- then the key/value data, then the data LEVEL BY LEVEL: a uint32 imageSize (the bytes of one face of a
 * cube map, of the whole level otherwise) followed by the level's 1 or 6 images in the order +X -X +Y -Y +Z -Z.  Level l is
 * max(1, w >> l) x max(1, h >> l) texels, ceil(w/4) x ceil(h/4) blocks of 8 bytes; every image is a multiple of 8 bytes, so the
 * format's cube and mip padding never occurs.
 *
 * FILE ORDER IS LEVEL-MAJOR, THEN FACE: image index = level * faces + face.  DDS, above, is face-major.  The images of a KTX
 * file are not one packed stream either -- a size word sits in front of each level -- so a loader copies them into one before
 * itwDecodeChain (itw_decode.h).
 *
 * Not here: KTX2, PKM, texture arrays, 3D textures (DDS has them, above), the other byte order, any other internal format.
 */
typedef struct ItwKtxDesc {
    uint32_t width, height;         /* level 0, texels; >= 1 */
    uint32_t mip_levels;            /* 1 .. 32 */
    uint32_t gl_internal_format;    /* 0x8D64 (ITW_FORMAT_ETC1_RGB8) */
    uint32_t is_cubemap;            /* 0 / 1: six faces, width == height */
    uint32_t key_value_bytes;       /* bytesOfKeyValueData: 0 in what this library writes; reported by itwKtxReadHeader and counted in every offset */
} ItwKtxDesc;

/* 64, the fixed header; 0 if `desc` is not a texture this library stores (see the struct). */
size_t itwKtxHeaderBytes(const ItwKtxDesc* desc);
/* header + key/value data + for every level its size word and images; 0 for a bad desc */
size_t itwKtxFileBytes(const ItwKtxDesc* desc);
/* Writes the 64 header bytes into dst; returns 64, or 0 on error (bad desc, key_value_bytes != 0, capacity < 64). */
size_t itwKtxWriteHeader(const ItwKtxDesc* desc, uint8_t* dst, size_t capacity);
/* Parses and checks a whole file's bytes; returns the offset of level 0's size word (64 + key_value_bytes), 0 for what this library
 * does not read: another identifier or byte order, an array, a depth, a height of 0, an internal format other than 0x8D64, faces other
 * than 1 or 6, a cube that is not square, more than 32 levels, a file shorter than itwKtxFileBytes, or one whose imageSize words
 * disagree with the sizes.  numberOfMipmapLevels 0 ("generate mips at load") reads as 1.  The key/value data is skipped. */
size_t itwKtxReadHeader(const uint8_t* src, size_t size, ItwKtxDesc* desc);
/* Whole file: `levels[i]` points at the blocks of image i in KTX order (level major, then face).  desc->key_value_bytes must be 0.
 * Returns bytes written (== itwKtxFileBytes) or 0. */
size_t itwKtxWriteFile(const ItwKtxDesc* desc, const uint8_t* const* levels, size_t nlevels, uint8_t* dst, size_t capacity);
/* Image `index` in KTX order (level * faces + face): its size in texels and the offset of its blocks from the start of the file.
 * Returns the image's byte size, 0 when index is out of range or desc is bad.  width, height and offset may each be NULL. */
size_t itwKtxImage(const ItwKtxDesc* desc, uint32_t index, uint32_t* width, uint32_t* height, size_t* offset);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
