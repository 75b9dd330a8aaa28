// bcn_format.hpp -- the block formats the decode side reads (decode_chain.hip, measure.hip, refine.hip), described once: the number a format
// goes by (the FMT template argument of the kernels), what a DXGI code maps to, the sizes that follow from it, and the one place where a
// runtime kind becomes a compile-time one.  Plain C++, no HIP headers: host-only programs use it too (tools/decode_chain_host_check.cpp).
// The encode side keeps its own switches (abi.hip job_of, GetBytesPerBlock with the reference's "unknown -> 8", dds.hip).
#pragma once
#include <cstdint>
#include <type_traits>
#include "../../include/ispc_texcomp.h"
#include "../../include/itw_dispatch.h"      // the format codes

namespace itw {

enum BcnKind : int { BCN_NONE = 0, BCN_BC1 = 1, BCN_BC3 = 3, BCN_BC4 = 4, BCN_BC5 = 5, BCN_BC6H = 6, BCN_BC7 = 7, BCN_BC4S = 14, BCN_BC5S = 15, BCN_ETC1 = 20 };

// DXGI format code (or ITW_FORMAT_ETC1_RGB8, ETC1's GL enum: it has no DXGI code) -> kind; BCN_NONE for what is not decoded.  BC6H_SF16 (96) reads as unsigned: the signed decode is not built, and the
// entry points that must not pretend otherwise (itwDecodeChain, itwDecodeImage) refuse 96 themselves.
constexpr int decode_kind(int dxgi)
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
    default: return BCN_NONE;
    }
}
constexpr int block_bytes(int kind) { return (kind == BCN_BC1 || kind == BCN_BC4 || kind == BCN_BC4S || kind == BCN_ETC1) ? 8 : 16; }
constexpr int texel_bytes(int kind) { return kind == BCN_BC6H ? 8 : 4; }                     // RGBA8 (int8 for the SNORM pair), RGBA16F
// the DirectXTex formats: their streams keep the partial blocks of a surface that is no multiple of 4 (itw_bc45.h)
constexpr bool keeps_partial_blocks(int kind) { return kind == BCN_BC4 || kind == BCN_BC5 || kind == BCN_BC4S || kind == BCN_BC5S; }
// the alpha code of a format whose decoder fills alpha in; -1 where alpha is decoded (BC1, BC3, BC7)
constexpr int filled_alpha(int kind)
{
    return (kind == BCN_BC4 || kind == BCN_BC5 || kind == BCN_ETC1) ? 255 : (kind == BCN_BC4S || kind == BCN_BC5S) ? 127 : kind == BCN_BC6H ? 0x3C00 : -1;
}
// the formats whose blocks have modes (decode_block's return value: 0 .. 15, or -1 for a block the format reserves); the others count as mode 0
constexpr bool has_modes(int kind) { return kind == BCN_BC7 || kind == BCN_BC6H || kind == BCN_ETC1; }
inline int64_t image_blocks(const rgba_surface& s) { return (((int64_t)s.width + 3) / 4) * (((int64_t)s.height + 3) / 4); }

// Calls f(std::integral_constant<int, kind>{}) for a kind decode_kind returned: with_kind(kind, [&](auto K) { launch<K.value>(...); })
template <class F>
inline void with_kind(int kind, F&& f)
{
    switch (kind) {
    case BCN_BC1:  f(std::integral_constant<int, BCN_BC1>{}); break;
    case BCN_BC3:  f(std::integral_constant<int, BCN_BC3>{}); break;
    case BCN_BC4:  f(std::integral_constant<int, BCN_BC4>{}); break;
    case BCN_BC5:  f(std::integral_constant<int, BCN_BC5>{}); break;
    case BCN_BC4S: f(std::integral_constant<int, BCN_BC4S>{}); break;
    case BCN_BC5S: f(std::integral_constant<int, BCN_BC5S>{}); break;
    case BCN_BC7:  f(std::integral_constant<int, BCN_BC7>{}); break;
    case BCN_BC6H: f(std::integral_constant<int, BCN_BC6H>{}); break;
    case BCN_ETC1: f(std::integral_constant<int, BCN_ETC1>{}); break;
    default: break;                                              // BCN_NONE: every entry point has refused it by now
    }
}

} // namespace itw
