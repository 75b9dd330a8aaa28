// preview_kernel_body.hpp -- the statements of preview.hip's viewport kernel, included into the body of each __global__ function that is one
// (preview_kernel<SRC, TILE>, preview_bc2_kernel<TILE>, preview_bc6hs_kernel<TILE>; preview.hip says why there are three).  Not a header in its own right: it expects
// `SRC` (a BcnKind or PREVIEW_RGBA8 / PREVIEW_RGBA16F), `TILE` and the kernel argument `const PreviewArgs a` in scope.
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
