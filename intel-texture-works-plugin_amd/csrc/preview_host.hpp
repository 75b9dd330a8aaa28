// preview_host.hpp -- the part of itwPreviewBlocks / itwPreviewSurface (preview.hip, include/itw_decode.h) that needs no device: the argument
// checks, the channel table, and the coordinate rule, which the kernel and the host share (the host needs it to know which rows of a host
// source the viewport can reach).  Plain C++, so that a host-only program can run it under a sanitizer (tools/preview_host_check.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "../../include/ispc_texcomp.h"
#include "../../include/itw_decode.h"
#include "bcn_format.hpp"

#ifdef __HIPCC__
#define ITW_PREVIEW_HD __host__ __device__ __forceinline__
#else
#define ITW_PREVIEW_HD inline
#endif

namespace itw {

// A workgroup of the tile route: 256 lanes, four consecutive pixels of a row each.
constexpr int PREVIEW_TILE_W = 64, PREVIEW_TILE_H = 16, PREVIEW_LANE_PIXELS = 4;
// Blocks across / down under n viewport pixels at `zoom`: the first and the last pixel's source coordinates lie less than (n - 1) * zoom + 1
// apart, so x1 - x0 <= ceil((n - 1) * zoom), and x0 can be the last texel of its block.
constexpr int preview_span_blocks(int n, double zoom)
{
    const double d = (n - 1) * zoom;
    const int whole = (int)d, texels = whole < d ? whole + 1 : whole;
    return (texels + 3) / 4 + 1;
}
// What the tile route's LDS holds: a tile's footprint at the largest zoom the route takes, 33 x 9 blocks at zoom 2 (two rounds of the 256
// lanes).  64 B a block (19 KB), 96 B for BC6H (28.5 KB).  The products are rounded, so a footprint can in principle come out one block
// larger at offsets near 2^30: the kernel counts every tile's footprint itself and one that does not fit takes the per-pixel route.
constexpr int PREVIEW_TILE_BLOCKS = preview_span_blocks(PREVIEW_TILE_W, ITW_PREVIEW_TILE_MAX_ZOOM) * preview_span_blocks(PREVIEW_TILE_H, ITW_PREVIEW_TILE_MAX_ZOOM);
static_assert(PREVIEW_TILE_BLOCKS == 33 * 9, "include/itw_decode.h states the footprint at ITW_PREVIEW_TILE_MAX_ZOOM");

// Step 1 of the definition: viewport coordinate t (xt or yt) with its offset -> source coordinate in 0 .. n - 1; false: outside.  The
// comparison comes before the conversion, so a product beyond the int range never reaches it.
ITW_PREVIEW_HD bool preview_coord(int t, int offset, double zoom, int n, int* x)
{
    const double f = (double)(t + offset) * zoom;
    if (f <= -1.0 || f >= (double)n) return false;
    *x = (int)f;                                                 // -1 < f < 0 truncates to 0
    return true;
}

// The source coordinates that viewport coordinates t0 .. t1 can show: the coordinate is monotone in t (an exact int -> double conversion, one
// multiply by a positive zoom, rounding is monotone), so they lie between those of the two ends.  false: none of them is inside.
ITW_PREVIEW_HD bool preview_range(int t0, int t1, int offset, double zoom, int n, int* lo, int* hi)
{
    const double f0 = (double)(t0 + offset) * zoom, f1 = (double)(t1 + offset) * zoom;
    if (f0 >= (double)n || f1 <= -1.0) return false;
    *lo = f0 <= -1.0 ? 0 : (int)f0;
    *hi = f1 >= (double)n ? n - 1 : (int)f1;
    return true;
}

// Step 3: the channel each output byte shows, 0 .. 3, or PREVIEW_NO_CHANNEL; *alpha_alone: the exposure is taken as 1.
constexpr int PREVIEW_NO_CHANNEL = 4;
inline void preview_channels(uint32_t options, int (&ch)[3], bool* alpha_alone)
{
    uint32_t m = options & ITW_PREVIEW_CHANNEL_MASK;
    if (!m) m = ITW_PREVIEW_CHANNEL_RED | ITW_PREVIEW_CHANNEL_GREEN | ITW_PREVIEW_CHANNEL_BLUE;
    *alpha_alone = m == ITW_PREVIEW_CHANNEL_ALPHA;
    const int single = m == ITW_PREVIEW_CHANNEL_RED ? 0 : m == ITW_PREVIEW_CHANNEL_GREEN ? 1 : m == ITW_PREVIEW_CHANNEL_BLUE ? 2 : m == ITW_PREVIEW_CHANNEL_ALPHA ? 3 : -1;
    if (single >= 0) { ch[0] = ch[1] = ch[2] = single; return; }
    ch[0] = (m & ITW_PREVIEW_CHANNEL_RED) ? 0 : PREVIEW_NO_CHANNEL;
    ch[1] = (m & ITW_PREVIEW_CHANNEL_GREEN) ? 1 : PREVIEW_NO_CHANNEL;
    ch[2] = (m & ITW_PREVIEW_CHANNEL_BLUE) ? 2 : PREVIEW_NO_CHANNEL;
    if (m & ITW_PREVIEW_CHANNEL_ALPHA) ch[2] = 3;                // the reference's channelIndex[2] = 3, whether or not blue is set
}

// The checks on the view and the output that both calls make before any device work.
inline bool preview_view_ok(const itw_preview_view* v, size_t view_bytes, const uint8_t* out_rgb, int64_t out_stride)
{
    if (!v || !out_rgb || view_bytes != sizeof(itw_preview_view)) return false;
    if (v->width < 1 || v->width > 16384 || v->height < 1 || v->height > 16384) return false;
    constexpr int32_t far = 1 << 30;
    if (v->x_offset < -far || v->x_offset > far || v->y_offset < -far || v->y_offset > far) return false;
    if (!std::isfinite(v->zoom) || !(v->zoom > 0.0)) return false;
    return out_stride >= (int64_t)3 * v->width;
}

// itwPreviewBlocks: BCN_NONE to refuse.  The SNORM pair decodes to texels the reference does not preview, and DXGI 96 stays refused: the signed
// reading of a BC6H stream is previewed under ITW_FORMAT_BC6H_SIGNED (the library's extension of the float route: itw_decode.h).
inline int preview_blocks_kind(int dxgi_format, const uint8_t* blocks, int width, int height)
{
    const int kind = dxgi_format == 96 ? BCN_NONE : decode_kind(stream_format(dxgi_format));      // (the BC1A codes: a BC1 stream)
    if (kind == BCN_NONE || kind == BCN_BC4S || kind == BCN_BC5S || !blocks || width < 1 || height < 1) return BCN_NONE;
    return image_blocks(rgba_surface{nullptr, width, height, 0}) > (int64_t)ITW_MEASURE_MAX_BLOCKS ? BCN_NONE : kind;
}

inline bool preview_surface_ok(const rgba_surface* s, int texel_bytes)
{
    if (!s || !s->ptr || (texel_bytes != 4 && texel_bytes != 8) || s->width < 1 || s->height < 1) return false;
    if ((int64_t)s->stride < (int64_t)s->width * texel_bytes) return false;
    return image_blocks(*s) <= (int64_t)ITW_MEASURE_MAX_BLOCKS;
}

} // namespace itw
