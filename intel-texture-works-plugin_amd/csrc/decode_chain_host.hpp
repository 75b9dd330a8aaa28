// decode_chain_host.hpp -- the part of itwDecodeChain (decode_chain.hip) that needs no device: format table, argument checks, the
// descriptor table and the staging layout.  Plain C++, so that a host-only program can run it under a sanitizer (tools/decode_chain_host_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/ispc_texcomp.h"
#include "../../include/itw_decode.h"

namespace itw {

// One image of a chain decode: where its texels go and where its blocks sit in the concatenated list.  first_block ascends with the index:
// the kernel finds a block's image by binary search, as chain_gather_kernel does over ChainImage.
struct DecodeImage { uint8_t* ptr; int64_t stride; int32_t width, height, blocks_x, _pad; int64_t first_block; };

// decode_kernel's FMT numbering; 0: not decoded by the chain entry points (BC6H_SF16 among them)
inline int decode_chain_kind(int f)
{
    return (f == 71 || f == 72) ? 1 : (f == 77 || f == 78) ? 3 : (f == 98 || f == 99) ? 7 : f == 95 ? 6 : f == 80 ? 4 : f == 83 ? 5 : f == 81 ? 14 : f == 84 ? 15 : 0;
}
inline int decode_chain_block_bytes(int kind) { return (kind == 1 || kind == 4 || kind == 14) ? 8 : 16; }
inline int decode_chain_texel_bytes(int kind) { return kind == 6 ? 8 : 4; }
inline int64_t decode_chain_blocks(const rgba_surface& s) { return (int64_t)((s.width + 3) / 4) * ((s.height + 3) / 4); }

// The checks of itwDecodeChain that come before any device work.  Returns the chain's block count (0 for count == 0), -1 to refuse.
inline int64_t decode_chain_check(int kind, const uint8_t* blocks, const rgba_surface* outs, int count)
{
    if (!kind || count < 0) return -1;
    if (count == 0) return 0;
    if (!blocks || !outs) return -1;
    const int64_t texel = decode_chain_texel_bytes(kind);
    int64_t total = 0;
    for (int i = 0; i < count; i++) {
        const rgba_surface& s = outs[i];
        if (!s.ptr || s.width < 1 || s.height < 1) return -1;
        if ((int64_t)s.stride < (int64_t)s.width * texel || (s.stride & 3)) return -1;
        const int64_t n = decode_chain_blocks(s);
        if (n > (int64_t)ITW_MEASURE_MAX_BLOCKS) return -1;
        total += n;
    }
    return total;
}

inline size_t decode_chain_up(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t decode_chain_pitch(int kind, const rgba_surface& s) { return ((size_t)s.width * (size_t)decode_chain_texel_bytes(kind) + 15) & ~(size_t)15; }

// Where each part of a call sits in the thread's device buffer: the table first, then whatever is staged for host pointers.
struct DecodeLayout { size_t desc, blocks, texels, modes, min_alpha, bytes; };

// Fills desc[0 .. count) and returns the layout.  With `stage_texels` image i decodes into the buffer (`base` + its offset, rows of
// decode_chain_pitch bytes, each image 256-B aligned) and not into outs[i].ptr; `base` may be null to size the buffer first.
inline DecodeLayout decode_chain_describe(int kind, const rgba_surface* outs, int count, int64_t total, uint8_t* base, bool stage_blocks,
                                          bool stage_texels, bool stage_modes, bool stage_min_alpha, DecodeImage* desc)
{
    DecodeLayout L{};
    size_t at = 0;
    L.desc = at;      at += decode_chain_up((size_t)count * sizeof(DecodeImage));
    L.blocks = at;    if (stage_blocks) at += decode_chain_up((size_t)total * (size_t)decode_chain_block_bytes(kind));
    L.modes = at;     if (stage_modes) at += decode_chain_up((size_t)total * 4);
    L.min_alpha = at; if (stage_min_alpha) at += decode_chain_up((size_t)count * 4);
    L.texels = at;
    int64_t first = 0;
    for (int i = 0; i < count; i++) {
        const rgba_surface& s = outs[i];
        DecodeImage& d = desc[i];
        if (stage_texels) {
            d.ptr = base ? base + at : nullptr;
            d.stride = (int64_t)decode_chain_pitch(kind, s);
            at += decode_chain_up((size_t)d.stride * (size_t)s.height);
        } else {
            d.ptr = s.ptr;
            d.stride = (int64_t)s.stride;
        }
        d.width = s.width; d.height = s.height;
        d.blocks_x = (s.width + 3) / 4; d._pad = 0;
        d.first_block = first;
        first += decode_chain_blocks(s);
    }
    L.bytes = at;
    return L;
}

} // namespace itw
