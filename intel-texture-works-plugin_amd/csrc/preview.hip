// preview.hip -- a viewport of an image, decoded where it is looked at (include/itw_decode.h: itwPreviewBlocks, itwPreviewSurface): what the
// reference's preview dialog asks of IntelPlugin::FetchPreviewRGB on every zoom, pan, channel toggle or exposure change.  The definition --
// coordinates, matte, channel table, tone -- is stated in the header; preview_host.hpp holds the part of it the host shares.
//
// One kernel, preview_kernel<SRC, TILE>.  A workgroup of 256 lanes owns a 64 x 16 tile of viewport pixels and a lane four consecutive pixels
// of one row: 12 bytes, which go out as three dwords where the row is dword aligned, and as bytes at the end of a row and in unaligned rows.
//   TILE (zoom <= ITW_PREVIEW_TILE_MAX_ZOOM): x and y are monotone in xt and yt, so the blocks under the tile are a rectangle known from
//     the tile's two corners.  Each is decoded once, one lane per block, by decode_core.hpp's decode_block into LDS, laid out [texel of the
//     block][block] so that neighbouring lanes write neighbouring banks; the pixels are then sampled from LDS.  At zoom 0.25 a decoded texel
//     is shown 16 times: the tile decodes about ten blocks where a decode per pixel would run 1024.  LDS holds the footprint at the largest
//     zoom of the route (preview_host.hpp: PREVIEW_TILE_BLOCKS); a tile that counts more blocks than that takes the other route.
//   otherwise: a lane decodes the block of its own pixel and keeps one texel, picked by sixteen compares (an index into the register array
//     that differs between lanes would send the array to scratch).
//     The RGBA8 / RGBA16F surfaces of itwPreviewSurface are this route with a plain load in place of the decode.
// Block and texel addresses are 64-bit.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/itw_decode.h"
#include "../../include/itw_amd.h"
#include "decode_core.hpp"
#include "preview_host.hpp"
#include "host_rt.hpp"

namespace itw {

// what a viewport is taken from: a block format (its BcnKind), or a surface of texels
enum : int { PREVIEW_RGBA8 = 100, PREVIEW_RGBA16F = 101 };
constexpr bool preview_is_surface(int src) { return src == PREVIEW_RGBA8 || src == PREVIEW_RGBA16F; }
constexpr bool preview_is_half(int src) { return src == PREVIEW_RGBA16F || src == BCN_BC6H; }

struct PreviewArgs {
    const uint8_t* src;          // block row / texel row `row0` of the image starts here (a host source is uploaded from that row on)
    int64_t src_stride;          // surfaces: bytes between texel rows
    int32_t width, height;       // the image
    int32_t blocks_x, row0;
    uint8_t* out;
    int64_t out_stride;
    int32_t view_w, view_h, x_offset, y_offset;
    double zoom;
    uint32_t matte;
    float exposure;              // 1 for alpha alone
    int32_t ch[3];               // channel of each output byte, 0 .. 3, or PREVIEW_NO_CHANNEL
};

// A texel as two dwords: RGBA8 in .x; RGBA16F as R | G << 16 in .x and B | A << 16 in .y
struct PreviewTexel { uint32_t x, y; };

// Step 4 of the definition for a half-float code: FloatToByte((float)half * exposure), the last product in double
__device__ __forceinline__ uint32_t preview_tone(uint32_t half_bits, float exposure)
{
    const uint16_t h = (uint16_t)half_bits;
    const float v = (float)__builtin_bit_cast(_Float16, h) * exposure;
    const double d = (double)v;
    if (d > 1.0) return 255u;
    if (!(d >= 0.0)) return 0u;                                  // negative, or NaN (-0.0 falls through to 0)
    return (uint32_t)(int)(d * 255.0);
}

template <bool HALF>
__device__ __forceinline__ uint32_t preview_byte(const PreviewTexel t, int ch, float exposure)
{
    if (ch == PREVIEW_NO_CHANNEL) return 0u;                     // (ch is a kernel argument: uniform)
    if (!HALF) return (t.x >> (8 * ch)) & 255u;
    return preview_tone(((ch < 2 ? t.x : t.y) >> (16 * (ch & 1))) & 0xffffu, exposure);
}

// Texel k of a decoded block held in registers, k differing between lanes: sixteen compares, never an indexed array.  The texels are OR-ed
// under a mask because the compiler folds a chain of `k == i ? px[i] : v` back into the indexed load px[k], which sends the array to scratch.
__device__ __forceinline__ uint32_t preview_pick(const uint32_t (&px)[16], int k)
{
    uint32_t v = 0u;
#pragma unroll
    for (int i = 0; i < 16; i++) v |= (k == i) ? px[i] : 0u;
    return v;
}

template <int SRC, bool TILE>
__global__ void __launch_bounds__(256) preview_kernel(const PreviewArgs a)
{
    constexpr bool HALF = preview_is_half(SRC);
    static_assert(!(TILE && preview_is_surface(SRC)), "a surface is sampled with plain loads");
    const int tid = threadIdx.x;
    const int xt0 = blockIdx.x * PREVIEW_TILE_W + (tid & 15) * PREVIEW_LANE_PIXELS, yt = blockIdx.y * PREVIEW_TILE_H + (tid >> 4);
    const bool row_live = yt < a.view_h && xt0 < a.view_w;
    int y = 0;
    const bool y_in = row_live && preview_coord(yt, a.y_offset, a.zoom, a.height, &y);

    // ---- the tile's footprint, decoded once into LDS ---------------------------------------------------------------------------------
    __shared__ uint32_t lds_lo[TILE ? 16 * PREVIEW_TILE_BLOCKS : 1];
    __shared__ uint16_t lds_hi[TILE && HALF ? 16 * PREVIEW_TILE_BLOCKS : 1];      // BC6H: blue; alpha is the constant 0x3C00
    bool staged = false;
    int bx0 = 0, by0 = 0, nbx = 0;
    if constexpr (TILE) {
        const int tx0 = blockIdx.x * PREVIEW_TILE_W, ty0 = blockIdx.y * PREVIEW_TILE_H;
        int xlo, xhi, ylo, yhi, nblocks = 0;
        if (preview_range(tx0, min(tx0 + PREVIEW_TILE_W, a.view_w) - 1, a.x_offset, a.zoom, a.width, &xlo, &xhi) &&
            preview_range(ty0, min(ty0 + PREVIEW_TILE_H, a.view_h) - 1, a.y_offset, a.zoom, a.height, &ylo, &yhi)) {
            bx0 = xlo >> 2; by0 = ylo >> 2;
            nbx = (xhi >> 2) - bx0 + 1;
            nblocks = nbx * ((yhi >> 2) - by0 + 1);              // <= 2^25: both factors are block counts of the image
        }
        staged = nblocks <= PREVIEW_TILE_BLOCKS;                 // uniform over the workgroup; an empty footprint counts as staged
        if (staged) {
            for (int b = tid; b < nblocks; b += 256) {
                const int ry = b / nbx, rx = b - ry * nbx;
                const int64_t j = (int64_t)(by0 + ry - a.row0) * a.blocks_x + (bx0 + rx);
                const uint4 w = load_block<SRC>(a.src, j);
                if constexpr (HALF) {
                    uint32_t lo[16], hi[16];
                    decode_block<SRC>(w, lo, hi);
#pragma unroll
                    for (int k = 0; k < 16; k++) { lds_lo[k * PREVIEW_TILE_BLOCKS + b] = lo[k]; lds_hi[k * PREVIEW_TILE_BLOCKS + b] = (uint16_t)hi[k]; }
                } else {
                    uint32_t px[16];
                    decode_block<SRC>(w, px);
#pragma unroll
                    for (int k = 0; k < 16; k++) lds_lo[k * PREVIEW_TILE_BLOCKS + b] = px[k];
                }
            }
            __syncthreads();
        }
    }

    // ---- this lane's four pixels ---------------------------------------------------------------------------------------------------
    const uint32_t matte = a.matte & 0xffffffu;
    uint32_t rgb[PREVIEW_LANE_PIXELS];
#pragma unroll 1
    for (int p = 0; p < PREVIEW_LANE_PIXELS; p++) {              // one copy of the decoder; p is uniform
        int x = 0;
        const bool in = y_in && xt0 + p < a.view_w && preview_coord(xt0 + p, a.x_offset, a.zoom, a.width, &x);
        PreviewTexel t{0u, 0u};
        if (in) {
            if constexpr (preview_is_surface(SRC)) {
                const uint8_t* q = a.src + (int64_t)(y - a.row0) * a.src_stride + (int64_t)x * (HALF ? 8 : 4);
                if constexpr (HALF) { const uint2 v = *reinterpret_cast<const uint2*>(q); t = PreviewTexel{v.x, v.y}; }
                else t.x = *reinterpret_cast<const uint32_t*>(q);
            } else {
                const int k = (y & 3) * 4 + (x & 3);
                if (staged) {
                    const int b = ((y >> 2) - by0) * nbx + ((x >> 2) - bx0);
                    t.x = lds_lo[k * PREVIEW_TILE_BLOCKS + b];
                    if constexpr (HALF) t.y = (uint32_t)lds_hi[k * PREVIEW_TILE_BLOCKS + b] | 0x3C000000u;
                } else {
                    const uint4 w = load_block<SRC>(a.src, (int64_t)((y >> 2) - a.row0) * a.blocks_x + (x >> 2));
                    if constexpr (HALF) {
                        uint32_t lo[16], hi[16];
                        decode_block<SRC>(w, lo, hi);
                        t = PreviewTexel{preview_pick(lo, k), preview_pick(hi, k)};
                    } else {
                        uint32_t px[16];
                        decode_block<SRC>(w, px);
                        t.x = preview_pick(px, k);
                    }
                }
            }
        }
        const uint32_t shown = preview_byte<HALF>(t, a.ch[0], a.exposure) | (preview_byte<HALF>(t, a.ch[1], a.exposure) << 8) |
                               (preview_byte<HALF>(t, a.ch[2], a.exposure) << 16);
        const uint32_t v = in ? shown : matte;
        rgb[0] = p == 0 ? v : rgb[0]; rgb[1] = p == 1 ? v : rgb[1]; rgb[2] = p == 2 ? v : rgb[2]; rgb[3] = p == 3 ? v : rgb[3];
    }
    if (!row_live) return;

    // ---- 12 bytes: three dwords, or bytes where the row's address or its end does not allow them ---------------------------------------
    uint8_t* o = a.out + (int64_t)yt * a.out_stride + (int64_t)xt0 * 3;
    const int n = min(PREVIEW_LANE_PIXELS, a.view_w - xt0);
    if (n == PREVIEW_LANE_PIXELS && ((uintptr_t)o & 3) == 0) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
        o4[0] = rgb[0] | (rgb[1] << 24);
        o4[1] = (rgb[1] >> 8) | (rgb[2] << 16);
        o4[2] = (rgb[2] >> 16) | (rgb[3] << 8);
    } else {
#pragma unroll
        for (int p = 0; p < PREVIEW_LANE_PIXELS; p++)
            if (p < n) { o[3 * p] = (uint8_t)rgb[p]; o[3 * p + 1] = (uint8_t)(rgb[p] >> 8); o[3 * p + 2] = (uint8_t)(rgb[p] >> 16); }
    }
}

} // namespace itw

namespace {

inline size_t preview_up(size_t v) { return (v + 255) & ~(size_t)255; }

// Everything that needs the device, for `who`.  src: PREVIEW_RGBA8 / PREVIEW_RGBA16F, or the BcnKind of `data`'s blocks; stride: a surface's.
void preview(const char* who, int src, const uint8_t* data, int64_t stride, int width, int height, const itw_preview_view& v, uint8_t* out_rgb,
             int64_t out_stride)
{
    hipStream_t st = (hipStream_t)itwGetStream();
    const bool surface = itw::preview_is_surface(src), dsrc = itw::is_device_pointer(data), dout = itw::is_device_pointer(out_rgb);
    const int texel = src == itw::PREVIEW_RGBA16F ? 8 : 4;
    if (dsrc && (surface ? (((uintptr_t)data | (uintptr_t)stride) & (uintptr_t)(texel - 1)) != 0 : ((uintptr_t)data & 3) != 0))
        itw::fail_msg("%s: device source at %p is not aligned to its %s", who, (const void*)data, surface ? "texels" : "dwords");

    itw::PreviewArgs a{};
    a.width = width; a.height = height; a.blocks_x = (width + 3) / 4;
    a.view_w = v.width; a.view_h = v.height; a.x_offset = v.x_offset; a.y_offset = v.y_offset; a.zoom = v.zoom;
    a.matte = v.matte_color;
    bool alpha_alone;
    int ch[3];
    itw::preview_channels(v.options, ch, &alpha_alone);
    for (int i = 0; i < 3; i++) a.ch[i] = ch[i];
    a.exposure = alpha_alone ? 1.0f : v.exposure;

    // a host source: the rows the viewport can reach, none if it misses the image; a host viewport: rows of a dword-aligned pitch
    int xlo, xhi, ylo = 0, yhi = -1;
    const bool reaches = itw::preview_range(0, v.width - 1, v.x_offset, v.zoom, width, &xlo, &xhi) &&
                         itw::preview_range(0, v.height - 1, v.y_offset, v.zoom, height, &ylo, &yhi);
    const int unit = surface ? 1 : 4;                            // rows of texels, or rows of blocks
    const int row0 = reaches ? ylo / unit : 0, rows = reaches ? yhi / unit - row0 + 1 : 0;
    const size_t src_pitch = surface ? (((size_t)width * texel + 15) & ~(size_t)15) : (size_t)a.blocks_x * (size_t)itw::block_bytes(src);
    const size_t src_bytes = dsrc ? 0 : preview_up(src_pitch * (size_t)rows), out_pitch = ((size_t)v.width * 3 + 3) & ~(size_t)3;
    const size_t out_bytes = dout ? 0 : out_pitch * (size_t)v.height;
    const bool resident = dsrc && dout;
    uint8_t* base = resident ? nullptr : static_cast<uint8_t*>(itw::decode_scratch(src_bytes + out_bytes + 256, st));

    a.src = data; a.src_stride = stride; a.row0 = 0;
    if (!dsrc) {
        a.src = base; a.src_stride = (int64_t)src_pitch; a.row0 = row0;
        if (rows > 0) {
            if (surface)
                ITW_CHECK(hipMemcpy2DAsync(base, src_pitch, data + (size_t)row0 * (size_t)stride, (size_t)stride, (size_t)width * texel, (size_t)rows,
                                           hipMemcpyHostToDevice, st));
            else
                ITW_CHECK(hipMemcpyAsync(base, data + (size_t)row0 * src_pitch, src_pitch * (size_t)rows, hipMemcpyHostToDevice, st));
        }
    }
    a.out = dout ? out_rgb : base + src_bytes;
    a.out_stride = dout ? out_stride : (int64_t)out_pitch;

    const dim3 grid((unsigned)((v.width + itw::PREVIEW_TILE_W - 1) / itw::PREVIEW_TILE_W), (unsigned)((v.height + itw::PREVIEW_TILE_H - 1) / itw::PREVIEW_TILE_H));
    if (src == itw::PREVIEW_RGBA8) hipLaunchKernelGGL((itw::preview_kernel<itw::PREVIEW_RGBA8, false>), grid, dim3(256), 0, st, a);
    else if (src == itw::PREVIEW_RGBA16F) hipLaunchKernelGGL((itw::preview_kernel<itw::PREVIEW_RGBA16F, false>), grid, dim3(256), 0, st, a);
    else
        itw::with_kind(src, [&](auto K) {
            if constexpr (K.value != itw::BCN_BC4S && K.value != itw::BCN_BC5S) {      // refused by the checks
                if (v.zoom <= ITW_PREVIEW_TILE_MAX_ZOOM) hipLaunchKernelGGL((itw::preview_kernel<K.value, true>), grid, dim3(256), 0, st, a);
                else hipLaunchKernelGGL((itw::preview_kernel<K.value, false>), grid, dim3(256), 0, st, a);
            }
        });
    ITW_CHECK(hipGetLastError());
    if (resident) return;                                        // all on the device: asynchronous on the thread's stream

    if (!dout)
        ITW_CHECK(hipMemcpy2DAsync(out_rgb, (size_t)out_stride, a.out, out_pitch, (size_t)v.width * 3, (size_t)v.height, hipMemcpyDeviceToHost, st));
    ITW_CHECK(hipStreamSynchronize(st));
    itw::decode_scratch_done(st);
}

} // namespace

extern "C" int itwPreviewBlocks(int dxgi_format, const uint8_t* blocks, int width, int height, const itw_preview_view* view, size_t view_bytes,
                                uint8_t* out_rgb, int64_t out_stride)
{
    const int kind = itw::preview_blocks_kind(dxgi_format, blocks, width, height);
    if (kind == itw::BCN_NONE || !itw::preview_view_ok(view, view_bytes, out_rgb, out_stride)) return -1;
    const itw_preview_view v = *view;
    const bool ok = itw::guarded([&] { preview("itwPreviewBlocks", kind, blocks, 0, width, height, v, out_rgb, out_stride); });
    return ok ? 0 : -1;
}

extern "C" int itwPreviewSurface(const rgba_surface* source, int texel_bytes, const itw_preview_view* view, size_t view_bytes, uint8_t* out_rgb,
                                 int64_t out_stride)
{
    if (!itw::preview_surface_ok(source, texel_bytes) || !itw::preview_view_ok(view, view_bytes, out_rgb, out_stride)) return -1;
    const itw_preview_view v = *view;
    const rgba_surface s = *source;
    const bool ok = itw::guarded([&] {
        preview("itwPreviewSurface", texel_bytes == 8 ? itw::PREVIEW_RGBA16F : itw::PREVIEW_RGBA8, s.ptr, s.stride, s.width, s.height, v, out_rgb, out_stride);
    });
    return ok ? 0 : -1;
}
