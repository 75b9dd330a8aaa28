// bcn_format.hpp -- the block formats, described once for both sides of the library: the encode host layer (abi.hip, dispatch.hip, multigpu.hip)
// and the decode side (decode_chain.hip, measure.hip, refine.hip).  The number a format goes by (the FMT template argument of the decode
// kernels, the `kind` of an encode Job), what a DXGI code maps to, the sizes that follow from it, the geometry of a surface in a format, and
// the one place where a runtime kind becomes a compile-time one.  Plain C++, no HIP headers: host-only programs use it too
// (tools/decode_chain_host_check.cpp).  What is NOT a table fact stays with its owner: GetBytesPerBlock's "unknown -> 8" (the reference's),
// dds.hip's header fields, which settings struct a format takes (abi.hip job_of).
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include "../../include/ispc_texcomp.h"
#include "../../include/itw_dispatch.h"      // the format codes

namespace itw {

enum BcnKind : int { BCN_NONE = 0, BCN_BC1 = 1, BCN_BC2 = 2, BCN_BC3 = 3, BCN_BC4 = 4, BCN_BC5 = 5, BCN_BC6H = 6, BCN_BC7 = 7, BCN_BC4S = 14, BCN_BC5S = 15, BCN_ETC1 = 20, BCN_BC1A = 21, BCN_BC6HS = 22, BCN_BC3DX = 23 };

// DXGI format code (or ITW_FORMAT_ETC1_RGB8, ETC1's GL enum: it has no DXGI code; or the two BC1A codes, GL enums likewise) -> kind; BCN_NONE
// for what the library neither encodes nor decodes.  BCN_BC1A is an ENCODE kind (DirectXTex's colour-key BC1 encoder: partial blocks kept, an
// itw_bc1a_settings); its stream is a BC1 stream, so the decode side never sees the kind: its entry points read a code through stream_format.
// BCN_BC2 (DirectXTex's D3DXEncodeBC2: partial blocks kept, the same itw_bc1a_settings) is both an encode and a decode kind, and goes by its two
// GL enums only: DXGI 74 / 75 stay BCN_NONE at every entry point that takes a format code (they appear inside DDS descriptors and headers alone).
// BCN_BC3DX (DirectXTex's D3DXEncodeBC3 under ITW_FORMAT_BC3_DXTEX[_SRGB]: 16 bytes, partial blocks kept, the same itw_bc1a_settings) is an ENCODE
// kind like BCN_BC1A: its stream is a BC3 stream, which the decode side reads as 77 / 78 through stream_format; 77 / 78 stay BCN_BC3, kernel.ispc's encoder.
// BC6H_SF16 (96) reads as unsigned here: the encoder is the reference's one BC6H encoder for both codes, and the entry points that must not
// pretend otherwise (itwDecodeChain, itwDecodeImage, itwPreviewBlocks) refuse 96 themselves.  The signed reading of a BC6H stream
// (D3DXDecodeBC6HS) goes by ITW_FORMAT_BC6H_SIGNED and is a DECODE kind only, BCN_BC6HS: format_kind, which every encode entry point asks, does
// not know the code (there is no signed encoder: refuse_signed_bc6h, host_rt.hpp, says so); decode_kind below does.
constexpr BcnKind format_kind(int dxgi)
{
    switch (dxgi) {
    case 71: case 72: return BCN_BC1;
    case 77: case 78: return BCN_BC3;
    case 80: return BCN_BC4;
    case 81: return BCN_BC4S;
    case 83: return BCN_BC5;
    case 84: return BCN_BC5S;
    case 95: case 96: return BCN_BC6H;
    case 98: case 99: return BCN_BC7;
    case ITW_FORMAT_ETC1_RGB8: return BCN_ETC1;
    case ITW_FORMAT_BC1A_UNORM: case ITW_FORMAT_BC1A_UNORM_SRGB: return BCN_BC1A;
    case ITW_FORMAT_BC2_UNORM: case ITW_FORMAT_BC2_UNORM_SRGB: return BCN_BC2;
    case ITW_FORMAT_BC3_DXTEX: case ITW_FORMAT_BC3_DXTEX_SRGB: return BCN_BC3DX;
    default: return BCN_NONE;
    }
}
// the code a stream is decoded, measured, previewed and stored under: the BC1A codes are synonyms of 71 / 72 there, the BC3_DXTEX codes of 77 / 78
constexpr int stream_format(int code)
{
    return code == ITW_FORMAT_BC1A_UNORM ? 71 : code == ITW_FORMAT_BC1A_UNORM_SRGB ? 72 : code == ITW_FORMAT_BC3_DXTEX ? 77 : code == ITW_FORMAT_BC3_DXTEX_SRGB ? 78 : code;
}
// what the decode, measure and preview entry points read a stream_format code as: format_kind, and the signed BC6H reading under its own code
constexpr BcnKind decode_kind(int code) { return code == ITW_FORMAT_BC6H_SIGNED ? BCN_BC6HS : format_kind(code); }
constexpr bool is_bc6h(int kind) { return kind == BCN_BC6H || kind == BCN_BC6HS; }           // either reading: 16-byte blocks to RGBA16F texels
constexpr int block_bytes(int kind) { return (kind == BCN_BC1 || kind == BCN_BC4 || kind == BCN_BC4S || kind == BCN_ETC1 || kind == BCN_BC1A) ? 8 : 16; }
constexpr int texel_bytes(int kind) { return is_bc6h(kind) ? 8 : 4; }                        // RGBA8 (int8 for the SNORM pair), RGBA16F
// the DirectXTex formats: their streams keep the partial blocks of a surface that is no multiple of 4 (itw_bc45.h)
constexpr bool keeps_partial_blocks(int kind) { return kind == BCN_BC4 || kind == BCN_BC5 || kind == BCN_BC4S || kind == BCN_BC5S || kind == BCN_BC1A || kind == BCN_BC2 || kind == BCN_BC3DX; }
// the alpha code of a format whose decoder fills alpha in; -1 where alpha is decoded (BC1, BC1A, BC2, BC3, BC7)
constexpr int filled_alpha(int kind)
{
    return (kind == BCN_BC4 || kind == BCN_BC5 || kind == BCN_ETC1) ? 255 : (kind == BCN_BC4S || kind == BCN_BC5S) ? 127 : is_bc6h(kind) ? 0x3C00 : -1;
}
// the formats whose blocks have modes (decode_block's return value: 0 .. 15, or -1 for a block the format reserves); the others count as mode 0
constexpr bool has_modes(int kind) { return kind == BCN_BC7 || is_bc6h(kind) || kind == BCN_ETC1; }
inline int64_t image_blocks(const rgba_surface& s) { return (((int64_t)s.width + 3) / 4) * (((int64_t)s.height + 3) / 4); }   // an image of a chain: padded to whole blocks, whatever the format

// A width x height surface as ONE ENCODE CALL sees it.  The ISPC formats drop partial blocks (kernel.ispc:600-601), the DirectXTex formats
// keep them (DirectXTexCompress.cpp:108-116): block counts, the texel rows and bytes per row a host surface is staged with, the stream's
// size, and the staging pitch -- tight, rows 16-byte aligned so that the kernels' vector load path applies.
struct SurfaceGeometry {
    int bx = 0, by = 0;                 // blocks across and down; empty(): nothing to encode (the reference's loops do not run either)
    int bpb = 0, texel_bytes = 0;
    size_t row_bytes = 0, rows = 0;     // what is read of the surface
    size_t out_bytes = 0, pitch = 0;
    bool empty() const { return bx <= 0 || by <= 0; }
    int64_t blocks() const { return empty() ? 0 : (int64_t)bx * by; }
};
inline SurfaceGeometry surface_geometry(int kind, int width, int height)
{
    const bool keep = keeps_partial_blocks(kind);
    SurfaceGeometry g;
    g.bx = keep ? (width > 0 ? (width + 3) / 4 : 0) : width / 4;
    g.by = keep ? (height > 0 ? (height + 3) / 4 : 0) : height / 4;
    g.bpb = block_bytes(kind);
    g.texel_bytes = texel_bytes(kind);
    if (g.empty()) return g;
    g.row_bytes = keep ? (size_t)width * g.texel_bytes : (size_t)g.bx * 4 * g.texel_bytes;
    g.rows = keep ? (size_t)height : (size_t)g.by * 4;
    g.out_bytes = (size_t)g.bx * g.by * g.bpb;
    g.pitch = (g.row_bytes + 15) & ~(size_t)15;
    return g;
}

// Calls f(std::integral_constant<int, kind>{}) for a kind format_kind returned: with_kind(kind, [&](auto K) { launch<K.value>(...); })
template <class F>
inline void with_kind(int kind, F&& f)
{
    switch (kind) {
    case BCN_BC1:  f(std::integral_constant<int, BCN_BC1>{}); break;
    case BCN_BC2:  f(std::integral_constant<int, BCN_BC2>{}); break;
    case BCN_BC3:  f(std::integral_constant<int, BCN_BC3>{}); break;
    case BCN_BC4:  f(std::integral_constant<int, BCN_BC4>{}); break;
    case BCN_BC5:  f(std::integral_constant<int, BCN_BC5>{}); break;
    case BCN_BC4S: f(std::integral_constant<int, BCN_BC4S>{}); break;
    case BCN_BC5S: f(std::integral_constant<int, BCN_BC5S>{}); break;
    case BCN_BC7:  f(std::integral_constant<int, BCN_BC7>{}); break;
    case BCN_BC6H: f(std::integral_constant<int, BCN_BC6H>{}); break;
    case BCN_BC6HS: f(std::integral_constant<int, BCN_BC6HS>{}); break;
    case BCN_ETC1: f(std::integral_constant<int, BCN_ETC1>{}); break;
    default: break;                                              // BCN_NONE: every entry point has refused it by now (BCN_BC1A, BCN_BC3DX: encode kinds, never decoded)
    }
}

} // namespace itw
