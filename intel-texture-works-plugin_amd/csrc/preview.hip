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
constexpr bool preview_is_half(int src) { return src == PREVIEW_RGBA16F || is_bc6h(src); }

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

// The kernel's statements are in preview_kernel_body.hpp (they use SRC, TILE and the argument `a`): the file is included into the two
// kernels below, so that each is compiled as the one __global__ function it was -- the same statements inlined from a shared __device__
// function compile to different code for every existing instantiation (preview_kernel<6, true>: 150 VGPRs for 123).
template <int SRC, bool TILE>
__global__ void __launch_bounds__(256) preview_kernel(const PreviewArgs a)
{
#include "preview_kernel_body.hpp"
}

// BC2 under a name of its own: tests/test_preview_cpu.py pins the set of preview_kernel<SRC, TILE> instantiations as it was before BC2
// (that file does not change), so the format's two kernels are not further members of that set; tests/test_bc2_cpu.py pins their resources.
template <bool TILE>
__global__ void __launch_bounds__(256) preview_bc2_kernel(const PreviewArgs a)
{
    constexpr int SRC = BCN_BC2;
#include "preview_kernel_body.hpp"
}

// The signed reading of BC6H likewise, for the same reason; tests/test_bc6hs_cpu.py pins the pair's resources.  The tile is the RGBA16F one
// (96 B a block), and step 4 of the definition shows a negative half, -Inf included, as 0.
template <bool TILE>
__global__ void __launch_bounds__(256) preview_bc6hs_kernel(const PreviewArgs a)
{
    constexpr int SRC = BCN_BC6HS;
#include "preview_kernel_body.hpp"
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
            if constexpr (K.value == itw::BCN_BC2) {
                if (v.zoom <= ITW_PREVIEW_TILE_MAX_ZOOM) hipLaunchKernelGGL((itw::preview_bc2_kernel<true>), grid, dim3(256), 0, st, a);
                else hipLaunchKernelGGL((itw::preview_bc2_kernel<false>), grid, dim3(256), 0, st, a);
            } else if constexpr (K.value == itw::BCN_BC6HS) {
                if (v.zoom <= ITW_PREVIEW_TILE_MAX_ZOOM) hipLaunchKernelGGL((itw::preview_bc6hs_kernel<true>), grid, dim3(256), 0, st, a);
                else hipLaunchKernelGGL((itw::preview_bc6hs_kernel<false>), grid, dim3(256), 0, st, a);
            } else if constexpr (K.value != itw::BCN_BC4S && K.value != itw::BCN_BC5S) {      // refused by the checks
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
