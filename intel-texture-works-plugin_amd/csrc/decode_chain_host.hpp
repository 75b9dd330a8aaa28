// decode_chain_host.hpp -- the part of itwDecodeChain and itwDecodeBlocks (decode_chain.hip) that needs no device: argument checks, the
// descriptor table and the staging layout (the formats themselves: bcn_format.hpp).  Plain C++, so that a host-only program can run it
// under a sanitizer (tools/decode_chain_host_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/ispc_texcomp.h"
#include "../../include/itw_decode.h"
#include "bcn_format.hpp"

namespace itw {

// One image of a chain decode: where its texels go and where its blocks sit in the concatenated list.  first_block ascends with the index:
// the kernel finds a block's image by binary search, as chain_gather_kernel does over ChainImage.
struct DecodeImage { uint8_t* ptr; int64_t stride; int32_t width, height, blocks_x, _pad; int64_t first_block; };

// The most blocks one image may have on the kernel's side: a block's index within its image is an int32 there.  The chain entry points
// stay far below it (ITW_MEASURE_MAX_BLOCKS); it is what bounds itwDecodeBlocks.
constexpr int64_t DECODE_IMAGE_MAX_BLOCKS = 0x7fffffff;

// The checks of itwDecodeChain that come before any device work.  Returns the chain's block count (0 for count == 0), -1 to refuse.
inline int64_t decode_chain_check(int kind, const uint8_t* blocks, const rgba_surface* outs, int count)
{
    if (!kind || count < 0) return -1;
    if (count == 0) return 0;
    if (!blocks || !outs) return -1;
    int64_t total = 0;
    for (int i = 0; i < count; i++) {
        const rgba_surface& s = outs[i];
        if (!s.ptr || s.width < 1 || s.height < 1) return -1;
        if ((int64_t)s.stride < (int64_t)s.width * texel_bytes(kind) || (s.stride & 3)) return -1;
        const int64_t n = image_blocks(s);
        if (n > (int64_t)ITW_MEASURE_MAX_BLOCKS) return -1;
        total += n;
    }
    return total;
}

// itwDecodeBlocks' own rules, all before any device work: whole blocks only except for the formats that keep partial ones, a stride that is
// a multiple of 4, at least the row and no more than an rgba_surface holds, and no more blocks than one image of a launch may have (the
// refusal is tested; the largest image that passes is 128 GiB of texels, which no test decodes).  Returns the block count, -1 to refuse.
inline int64_t decode_blocks_check(int kind, int width, int height, int64_t out_stride)
{
    if (!kind || (out_stride & 3)) return -1;
    if (keeps_partial_blocks(kind) ? (width < 1 || height < 1) : (width < 4 || height < 4 || (width & 3) || (height & 3))) return -1;
    if (out_stride < (int64_t)width * texel_bytes(kind) || out_stride > (int64_t)INT32_MAX) return -1;
    const int64_t n = image_blocks(rgba_surface{nullptr, width, height, 0});
    return n > DECODE_IMAGE_MAX_BLOCKS ? -1 : n;
}

inline size_t decode_chain_up(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t decode_chain_pitch(int kind, const rgba_surface& s) { return ((size_t)s.width * (size_t)texel_bytes(kind) + 15) & ~(size_t)15; }

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
    L.blocks = at;    if (stage_blocks) at += decode_chain_up((size_t)total * (size_t)block_bytes(kind));
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
        first += image_blocks(s);
    }
    L.bytes = at;
    return L;
}

} // namespace itw
