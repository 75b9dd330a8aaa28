// decode_core.hpp -- BCn block decoding for gfx950, shared by everything that turns block words into texels: decode_chain.hip (blocks ->
// texels in memory), measure.hip and refine.hip (blocks -> registers -> error sums).  decode_block<FMT> is the one block -> 16 texels
// function; under it the per-format decoders (decode_color, decode_scalar_block, decode_bc7, decode_bc6h) and their tables.  Pure integer
// work.  Written from the format definitions (the readable statement inside the reference tree is its decoder: BC.cpp for BC1/BC3,
// BC4BC5.cpp for BC4/BC5, BC6HBC7.cpp:35-37 weights, :40 partitions, :247 fix-ups, :537 BC7 mode table, :1937-2140 BC7 decode,
// :310-500 BC6H mode descriptors, :1077-1235 BC6H decode, unsigned and signed, :1313-1359 unquantisation).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bc6h_layout.hpp"
#include "bcn_format.hpp"

namespace itw {

#define BCN_TABLE_QUAL __device__ const
namespace dec {
#include "bc7_tables.h"
}
#undef BCN_TABLE_QUAL

__device__ const Bc6hLayout D_BC6H_LAYOUT[14] = {
    BC6H_LAYOUT[0], BC6H_LAYOUT[1], BC6H_LAYOUT[2], BC6H_LAYOUT[3], BC6H_LAYOUT[4], BC6H_LAYOUT[5], BC6H_LAYOUT[6],
    BC6H_LAYOUT[7], BC6H_LAYOUT[8], BC6H_LAYOUT[9], BC6H_LAYOUT[10], BC6H_LAYOUT[11], BC6H_LAYOUT[12], BC6H_LAYOUT[13]};

__device__ const unsigned char D_WEIGHTS[3][16] = {
    {0, 21, 43, 64}, {0, 9, 18, 27, 37, 46, 55, 64}, {0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64}};

// LSB-first reader over a 128-bit block
struct Bits {
    unsigned long long lo, hi;
    int pos;
    __device__ __forceinline__ uint32_t take(int n)
    {
        if (n == 0) return 0u;
        unsigned long long v;
        if (pos >= 64) v = hi >> (pos - 64);
        else v = (lo >> pos) | (pos ? (hi << (64 - pos)) : 0ull);
        pos += n;
        return (uint32_t)(v & ((1ull << n) - 1ull));
    }
};

// ---- BC1 colour block; punch-through (3-colour) mode only where the format allows it ----------------------
__device__ __forceinline__ void decode_color(uint32_t w0, uint32_t idx, bool allow3, uint32_t (&px)[16])
{
    const uint32_t c0 = w0 & 0xffffu, c1 = w0 >> 16;
    int pal[4][3];
    const uint32_t c[2] = {c0, c1};
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int r = (c[i] >> 11) & 31, g = (c[i] >> 5) & 63, b = c[i] & 31;
        pal[i][0] = (r << 3) | (r >> 2); pal[i][1] = (g << 2) | (g >> 4); pal[i][2] = (b << 3) | (b >> 2);
    }
    const bool four = c0 > c1 || !allow3;
    uint32_t a2 = 255u, a3 = 255u;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        pal[2][ch] = four ? (2 * pal[0][ch] + pal[1][ch] + 1) / 3 : (pal[0][ch] + pal[1][ch]) / 2;
        pal[3][ch] = four ? (pal[0][ch] + 2 * pal[1][ch] + 1) / 3 : 0;
    }
    if (!four) a3 = 0u;
    uint32_t packed[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
        packed[i] = (uint32_t)pal[i][0] | ((uint32_t)pal[i][1] << 8) | ((uint32_t)pal[i][2] << 16) | ((i == 3 ? a3 : (i == 2 ? a2 : 255u)) << 24);
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t q = (idx >> (2 * k)) & 3u;
        px[k] = q == 0 ? packed[0] : q == 1 ? packed[1] : q == 2 ? packed[2] : packed[3];
    }
}

// The 8-byte interpolated-scalar block shared by BC3 alpha, BC4 and both halves of BC5; the value lands in byte SHIFT/8.
template <int SHIFT>
__device__ __forceinline__ void decode_scalar_block(uint32_t w0, uint32_t w1, uint32_t (&px)[16])
{
    int a[8];
    a[0] = (int)(w0 & 255u); a[1] = (int)((w0 >> 8) & 255u);
    if (a[0] > a[1]) {
#pragma unroll
        for (int i = 1; i < 7; i++) a[1 + i] = ((7 - i) * a[0] + i * a[1] + 3) / 7;
    } else {
#pragma unroll
        for (int i = 1; i < 5; i++) a[1 + i] = ((5 - i) * a[0] + i * a[1] + 2) / 5;
        a[6] = 0; a[7] = 255;
    }
    const unsigned long long bits = ((unsigned long long)(w0 >> 16)) | ((unsigned long long)w1 << 16);
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t q = (uint32_t)(bits >> (3 * k)) & 7u;
        int v = a[0];
#pragma unroll
        for (int i = 1; i < 8; i++) v = (q == (uint32_t)i) ? a[i] : v;
        px[k] = (px[k] & ~(0xffu << SHIFT)) | ((uint32_t)v << SHIFT);
    }
}
// The same block with signed endpoints (BC4_SNORM, both halves of BC5_SNORM): int8 values, endpoint -128 read as -127 for the values while
// the RAW bytes choose the form (BC4_SNORM::DecodeFromIndex, BC4BC5.cpp:106-131); levels 6 and 7 of the 6-level form are -127 and 127.
// round(n / d) to nearest = floor((2n + d) / (2d)), n offset by 128 * d so that the division works on a non-negative number.
template <int SHIFT>
__device__ __forceinline__ void decode_scalar_block_snorm(uint32_t w0, uint32_t w1, uint32_t (&px)[16])
{
    const int r0 = (int)(int8_t)(w0 & 255u), r1 = (int)(int8_t)((w0 >> 8) & 255u);
    int a[8];
    a[0] = r0 == -128 ? -127 : r0; a[1] = r1 == -128 ? -127 : r1;
    if (r0 > r1) {
#pragma unroll
        for (int i = 1; i < 7; i++) a[1 + i] = (2 * ((7 - i) * a[0] + i * a[1]) + 7 + 128 * 14) / 14 - 128;
    } else {
#pragma unroll
        for (int i = 1; i < 5; i++) a[1 + i] = (2 * ((5 - i) * a[0] + i * a[1]) + 5 + 128 * 10) / 10 - 128;
        a[6] = -127; a[7] = 127;
    }
    const unsigned long long bits = ((unsigned long long)(w0 >> 16)) | ((unsigned long long)w1 << 16);
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t q = (uint32_t)(bits >> (3 * k)) & 7u;
        int v = a[0];
#pragma unroll
        for (int i = 1; i < 8; i++) v = (q == (uint32_t)i) ? a[i] : v;
        px[k] = (px[k] & ~(0xffu << SHIFT)) | (((uint32_t)v & 0xffu) << SHIFT);
    }
}
__device__ __forceinline__ void decode_bc3_alpha(uint32_t w0, uint32_t w1, uint32_t (&px)[16]) { decode_scalar_block<24>(w0, w1, px); }

// ---- BC7 ---------------------------------------------------------------------------------------------------
struct Bc7Mode { unsigned char ns, pb, rb, isb, cb, ab, epb, spb, ib, ib2; };
__device__ const Bc7Mode D_BC7_MODES[8] = {
    {3, 4, 0, 0, 4, 0, 1, 0, 3, 0}, {2, 6, 0, 0, 6, 0, 0, 1, 3, 0}, {3, 6, 0, 0, 5, 0, 0, 0, 2, 0}, {2, 6, 0, 0, 7, 0, 1, 0, 2, 0},
    {1, 0, 2, 1, 5, 6, 0, 0, 2, 3}, {1, 0, 2, 0, 7, 8, 0, 0, 2, 2}, {1, 0, 0, 0, 7, 7, 1, 0, 4, 0}, {2, 6, 0, 0, 5, 5, 1, 0, 2, 0}};

__device__ __forceinline__ int decode_bc7(Bits& bs, uint32_t (&px)[16])
{
    int mode = 0;
    while (mode < 8 && !bs.take(1)) mode++;
    if (mode == 8) {
#pragma unroll
        for (int k = 0; k < 16; k++) px[k] = 0u;
        return -1;
    }
    const Bc7Mode mi = D_BC7_MODES[mode];
    const int shape = (int)bs.take(mi.pb), rot = (int)bs.take(mi.rb), isel = (int)bs.take(mi.isb);
    int ep[6][4];
    for (int ch = 0; ch < 3; ch++)
        for (int e = 0; e < 6; e++) ep[e][ch] = (e < mi.ns * 2) ? (int)bs.take(mi.cb) : 0;
    for (int e = 0; e < 6; e++) ep[e][3] = (e < mi.ns * 2 && mi.ab) ? (int)bs.take(mi.ab) : 255;
    int cbits = mi.cb, abits = mi.ab;
    if (mi.epb) {
        for (int e = 0; e < 6; e++)
            if (e < mi.ns * 2) {
                const int p = (int)bs.take(1);
                for (int ch = 0; ch < 3; ch++) ep[e][ch] = (ep[e][ch] << 1) | p;
                if (mi.ab) ep[e][3] = (ep[e][3] << 1) | p;
            }
        cbits++; if (mi.ab) abits++;
    } else if (mi.spb) {
        for (int s = 0; s < 3; s++)
            if (s < mi.ns) {
                const int p = (int)bs.take(1);
                for (int e = 2 * s; e < 2 * s + 2; e++)
                    for (int ch = 0; ch < 3; ch++) ep[e][ch] = (ep[e][ch] << 1) | p;
            }
        cbits++;
    }
    for (int e = 0; e < 6; e++) {
        for (int ch = 0; ch < 3; ch++) { const int v = ep[e][ch] << (8 - cbits); ep[e][ch] = v | (v >> cbits); }
        if (mi.ab) { const int v = ep[e][3] << (8 - abits); ep[e][3] = v | (v >> abits); }
    }
    const int table = (mi.ns == 3) ? 64 + shape : shape;
    const uint32_t pattern = (mi.ns == 1) ? 0u : dec::BCN_PATTERN[table];
    const int anc1 = (mi.ns >= 2) ? (dec::BCN_ANCHORS[table] >> 4) : 0, anc2 = (mi.ns >= 2) ? (dec::BCN_ANCHORS[table] & 15) : 0;
    uint32_t i1[2] = {0u, 0u}, i2[2] = {0u, 0u};          // 4 bits per texel
    for (int k = 0; k < 16; k++) {
        const int sub = (int)((pattern >> (2 * k)) & 3u);
        const int anchor = sub == 0 ? 0 : (sub == 1 ? anc1 : anc2);
        const uint32_t v = bs.take(mi.ib - (k == anchor ? 1 : 0));
        i1[k >> 3] |= v << (4 * (k & 7));
    }
    if (mi.ib2)
        for (int k = 0; k < 16; k++) i2[k >> 3] |= bs.take(mi.ib2 - (k == 0 ? 1 : 0)) << (4 * (k & 7));
    for (int k = 0; k < 16; k++) {
        const int sub = (int)((pattern >> (2 * k)) & 3u);
        int ci = (int)((i1[k >> 3] >> (4 * (k & 7))) & 15u), ai = ci, cbw = mi.ib, abw = mi.ib;
        if (mi.ib2) {
            const int second = (int)((i2[k >> 3] >> (4 * (k & 7))) & 15u);
            if (isel) { ci = second; cbw = mi.ib2; } else { ai = second; abw = mi.ib2; }
        }
        const int wc = D_WEIGHTS[cbw - 2][ci], wa = D_WEIGHTS[abw - 2][ai];
        int v[4];
        for (int ch = 0; ch < 4; ch++) {
            int e0 = 0, e1 = 0;
            for (int s = 0; s < 3; s++) if (s == sub) { e0 = ep[2 * s][ch]; e1 = ep[2 * s + 1][ch]; }
            const int w = (ch == 3) ? wa : wc;
            v[ch] = (e0 * (64 - w) + e1 * w + 32) >> 6;
        }
        if (!mi.ab) v[3] = 255;
        if (rot == 1) { const int t = v[3]; v[3] = v[0]; v[0] = t; }
        else if (rot == 2) { const int t = v[3]; v[3] = v[1]; v[1] = t; }
        else if (rot == 3) { const int t = v[3]; v[3] = v[2]; v[2] = t; }
        px[k] = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    }
    return mode;
}

// ---- BC6H, unsigned and signed -----------------------------------------------------------------------------
__device__ __forceinline__ int unquantize_uf16(int comp, int bits)
{
    if (bits >= 15) return comp;
    if (comp == 0) return 0;
    if (comp == ((1 << bits) - 1)) return 0xFFFF;
    return ((comp << 16) + 0x8000) >> bits;
}
// SIGN_EXTEND (BC.h:33): bit nb - 1 of a field of nb bits is its sign
__device__ __forceinline__ int sign_extend(int x, int nb) { return (x & (1 << (nb - 1))) ? (x | ~((1 << nb) - 1)) : x; }
// Unquantize(comp, bits, true) (BC6HBC7.cpp:1316-1335): on the magnitude, the sign put back at the end
__device__ __forceinline__ int unquantize_sf16(int comp, int bits)
{
    if (bits >= 16) return comp;
    const int m = comp < 0 ? -comp : comp;
    const int unq = m == 0 ? 0 : m >= ((1 << (bits - 1)) - 1) ? 0x7FFF : ((m << 15) + 0x4000) >> (bits - 1);
    return comp < 0 ? -unq : unq;
}
// FinishUnquantize(x, true) (:1351-1354), then INT2F16(.., true) (BC.h:407-420): sign bit | magnitude, no clamp, zero never -0.  An endpoint of
// -32768 (the 16-bit mode alone) can interpolate to -32768: (32768 * 31) >> 5 = 0x7C00 under the sign bit, -Inf; the largest positive value is 0x7BFF.
__device__ __forceinline__ uint32_t finish_sf16(int x)
{
    const int f = x < 0 ? -(((-x) * 31) >> 5) : (x * 31) >> 5;      // (a small negative x finishes as 0, which takes no sign bit)
    return f < 0 ? (0x8000u | (uint32_t)(-f)) : (uint32_t)f;
}

// SIGNED: D3DXDecodeBC6HS (D3DX_BC6H::Decode(true, ..), :1077-1235) -- endpoint 0.A sign-extended at the base precision and every other endpoint
// at its own field width, in transformed and untransformed modes alike (:1143-1159); TransformInverse masks the sum and sign-extends it again at
// the base precision (:582-594); interpolation on signed ints with an arithmetic shift.  The unsigned reading is every `if constexpr (!SIGNED)` branch.
template <bool SIGNED = false>
__device__ __forceinline__ int decode_bc6h(Bits& bs, uint32_t (&lo)[16], uint32_t (&hi)[16])
{
    int m = (int)bs.take(2);
    if (m >= 2) m |= (int)bs.take(3) << 2;
    int mode = -1;
    for (int i = 0; i < 14; i++) if (D_BC6H_LAYOUT[i].prefix == m) mode = i;
    if (mode < 0) {
#pragma unroll
        for (int k = 0; k < 16; k++) { lo[k] = 0u; hi[k] = 0x3C000000u; }
        return -1;
    }
    const Bc6hLayout& L = D_BC6H_LAYOUT[mode];
    int e[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    int shape = 0;
    const int header = L.two_regions ? 82 : 65;
    while (bs.pos < header) {
        const int cur = bs.pos;
        if (bs.take(1)) {
            const int field = L.slot[cur] >> 4, bit = L.slot[cur] & 15;
            if (field == 2) shape |= 1 << bit;
            else if (field >= 3) {
                const int f = field - 3, which = f & 3, ch = f >> 2;
                for (int a = 0; a < 4; a++) for (int c = 0; c < 3; c++) if (a == which && c == ch) e[a][c] |= 1 << bit;
            }
        }
    }
    if constexpr (!SIGNED) {
        if (L.transformed)
            for (int ch = 0; ch < 3; ch++) {
                const int mask = (1 << L.base_bits[ch]) - 1, db = L.delta_bits[ch];
                for (int k = 1; k < 4; k++)
                    if (k < (L.two_regions ? 4 : 2)) {
                        const int d = (e[k][ch] & (1 << (db - 1))) ? (e[k][ch] | ~((1 << db) - 1)) : e[k][ch];
                        e[k][ch] = (d + e[0][ch]) & mask;
                    }
            }
    } else {
        for (int ch = 0; ch < 3; ch++) {
            const int bb = L.base_bits[ch], db = L.delta_bits[ch];       // delta_bits: the field's width, = base_bits in the untransformed modes
            e[0][ch] = sign_extend(e[0][ch], bb);
            for (int k = 1; k < 4; k++)
                if (k < (L.two_regions ? 4 : 2)) {
                    const int d = sign_extend(e[k][ch], db);
                    e[k][ch] = L.transformed ? sign_extend((d + e[0][ch]) & ((1 << bb) - 1), bb) : d;
                }
        }
    }
    const int ib = L.two_regions ? 3 : 4;
    const uint32_t pattern = L.two_regions ? dec::BCN_PATTERN[shape] : 0u;
    const int anchor1 = L.two_regions ? (dec::BCN_ANCHORS[shape] >> 4) : -1;
    for (int k = 0; k < 16; k++) {
        const int region = (int)((pattern >> (2 * k)) & 3u);
        const int n = ib - ((k == 0 || (region == 1 && k == anchor1)) ? 1 : 0);
        const int w = D_WEIGHTS[ib - 2][bs.take(n)];
        if constexpr (!SIGNED) {
            int v[3];
            for (int ch = 0; ch < 3; ch++) {
                const int a = unquantize_uf16(region ? e[2][ch] : e[0][ch], L.base_bits[ch]);
                const int b = unquantize_uf16(region ? e[3][ch] : e[1][ch], L.base_bits[ch]);
                int x = (a * (64 - w) + b * w + 32) >> 6;
                x = (x * 31) >> 6;
                v[ch] = x > 0x7BFF ? 0x7BFF : x;
            }
            lo[k] = (uint32_t)v[0] | ((uint32_t)v[1] << 16);
            hi[k] = (uint32_t)v[2] | 0x3C000000u;
        } else {
            uint32_t v[3];
            for (int ch = 0; ch < 3; ch++) {
                const int a = unquantize_sf16(region ? e[2][ch] : e[0][ch], L.base_bits[ch]);
                const int b = unquantize_sf16(region ? e[3][ch] : e[1][ch], L.base_bits[ch]);
                v[ch] = finish_sf16((a * (64 - w) + b * w + 32) >> 6);
            }
            lo[k] = v[0] | (v[1] << 16);
            hi[k] = v[2] | 0x3C000000u;
        }
    }
    return mode;
}

// ---- ETC1 (OES_compressed_ETC1_RGB8_texture) -----------------------------------------------------------------------------------------------
// Bytes 0-2: the two base colours per channel -- individual: two 4-bit values (first sub-block in the high nibble), each x 17; differential: a
// 5-bit base and a 3-bit signed delta, each 5-bit value v extended (v << 3) | (v >> 2).  Byte 3: table of sub-block 0 in bits 7-5, of sub-block
// 1 in bits 4-2, diff in bit 1, flip in bit 0.  Bytes 4-7: the MSB and the LSB plane of the selectors, big-endian, texel (x, y) at bit x * 4 + y.
// flip 0: sub-block 1 is columns 2-3; flip 1: rows 2-3.  Returns the mode: 0 individual, 1 differential, -1 for a differential block whose
// base + delta leaves 0 .. 31 (invalid in ETC1; decoded with the sum modulo 32).
__device__ const unsigned char D_ETC1_MODIFIERS[8][2] = {{2, 8}, {5, 17}, {9, 29}, {13, 42}, {18, 60}, {24, 80}, {33, 106}, {47, 183}};

__device__ __forceinline__ int decode_etc1(uint32_t w0, uint32_t w1, uint32_t (&px)[16])
{
    const bool flip = (w0 >> 24) & 1u, diff = (w0 >> 25) & 1u;
    const int table[2] = {(int)((w0 >> 29) & 7u), (int)((w0 >> 26) & 7u)};
    int base[2][3];
    bool overflow = false;
#pragma unroll
    for (int p = 0; p < 3; p++) {
        const int byte = (int)((w0 >> (8 * p)) & 255u);
        if (diff) {
            const int v = byte >> 3, d = (byte & 7) - ((byte & 4) << 1), sum = v + d;
            overflow = overflow || sum < 0 || sum > 31;
            const int u = sum & 31;
            base[0][p] = (v << 3) | (v >> 2);
            base[1][p] = (u << 3) | (u >> 2);
        } else {
            base[0][p] = (byte >> 4) * 17;
            base[1][p] = (byte & 15) * 17;
        }
    }
    const uint32_t planes = __builtin_bswap32(w1);              // MSB plane in the high half, LSB plane in the low half
    int small[2], large[2];
#pragma unroll
    for (int i = 0; i < 2; i++) { small[i] = D_ETC1_MODIFIERS[table[i]][0]; large[i] = D_ETC1_MODIFIERS[table[i]][1]; }
#pragma unroll
    for (int y = 0; y < 4; y++)
#pragma unroll
        for (int x = 0; x < 4; x++) {
            const int bit = x * 4 + y, sub = flip ? (y >> 1) : (x >> 1);
            const bool msb = (planes >> (16 + bit)) & 1u, lsb = (planes >> bit) & 1u;
            const int mag = lsb ? (sub ? large[1] : large[0]) : (sub ? small[1] : small[0]), m = msb ? -mag : mag;
            uint32_t texel = 255u << 24;
#pragma unroll
            for (int p = 0; p < 3; p++) texel |= (uint32_t)min(max((sub ? base[1][p] : base[0][p]) + m, 0), 255) << (8 * p);
            px[y * 4 + x] = texel;
        }
    return overflow ? -1 : (diff ? 1 : 0);
}

// ---- any format: block words -> 16 texels -------------------------------------------------------------------------------------------
// the 128 bits of a block as the LSB-first reader takes them
__device__ __forceinline__ Bits block_bits(const uint4 w)
{
    return Bits{(unsigned long long)w.x | ((unsigned long long)w.y << 32), (unsigned long long)w.z | ((unsigned long long)w.w << 32), 0};
}

// Decodes the block whose words are `w` (the 8-byte formats use .x and .y) into RGBA8 dwords (int8 codes for the SNORM pair) and returns
// its mode: BC7 0..7 or -1 for the reserved prefix, ETC1 0 / 1 or -1 (decode_etc1), 0 for the formats without modes.  Alpha is filled where the format has none
// (filled_alpha): BC4 / BC5 decode to (R, 0, 0, 255) / (R, G, 0, 255) like D3DXDecodeBC4U / BC5U (BC4BC5.cpp:373-385, 449-462), their
// SNORM forms to int8 (R, 0, 0, 127) / (R, G, 0, 127) (:388-400, :465-478).
template <int FMT>
__device__ __forceinline__ int decode_block(const uint4 w, uint32_t (&px)[16])
{
    static_assert(!is_bc6h(FMT), "BC6H decodes to RGBA16F: the overload below");
    if (FMT == BCN_BC7) {
        Bits bs = block_bits(w);
        return decode_bc7(bs, px);
    } else if (FMT == BCN_ETC1) {
        return decode_etc1(w.x, w.y, px);
    } else if (FMT == BCN_BC1) {
        decode_color(w.x, w.y, true, px);
    } else if (FMT == BCN_BC3) {
        decode_color(w.z, w.w, false, px);
        decode_bc3_alpha(w.x, w.y, px);
    } else if (FMT == BCN_BC2) {
        decode_color(w.z, w.w, false, px);            // always the four-colour palette, whatever the order of the endpoints (D3DXDecodeBC2, BC.cpp:802)
#pragma unroll
        for (int k = 0; k < 16; k++)                  // texel k: nibble k & 7 of word k >> 3; a 4-bit code n is n * 17 (= n / 15 of 255, exactly)
            px[k] = (px[k] & 0x00ffffffu) | ((((k < 8 ? w.x : w.y) >> (4 * (k & 7))) & 15u) * 17u << 24);
    } else {
        constexpr bool SNORM = FMT == BCN_BC4S || FMT == BCN_BC5S;
#pragma unroll
        for (int k = 0; k < 16; k++) px[k] = (uint32_t)filled_alpha(FMT) << 24;
        if (SNORM) decode_scalar_block_snorm<0>(w.x, w.y, px); else decode_scalar_block<0>(w.x, w.y, px);
        if (FMT == BCN_BC5) decode_scalar_block<8>(w.z, w.w, px);
        if (FMT == BCN_BC5S) decode_scalar_block_snorm<8>(w.z, w.w, px);
    }
    return 0;
}
// BC6H, either reading: the two dwords of each RGBA16F texel, lo = R | G << 16, hi = B | A << 16 with alpha 1.0; mode 0..13, -1 for a reserved prefix
template <int FMT>
__device__ __forceinline__ int decode_block(const uint4 w, uint32_t (&lo)[16], uint32_t (&hi)[16])
{
    static_assert(is_bc6h(FMT), "the RGBA8 formats: the overload above");
    Bits bs = block_bits(w);
    return decode_bc6h<FMT == BCN_BC6HS>(bs, lo, hi);
}

// Block j of a stream whose base is 16-byte aligned (8 for the 8-byte formats) or only 4-byte aligned (the payload of a DDS file).  Callers
// that guarantee the alignment (measure.hip, refine.hip) load the vector themselves and carry no branch.
template <int FMT>
__device__ __forceinline__ uint4 load_block(const uint8_t* __restrict__ blocks, int64_t j)
{
    if constexpr (block_bytes(FMT) == 8) {
        const uint8_t* p = blocks + j * 8;
        if (((uintptr_t)p & 7) == 0) { const uint2 v = *reinterpret_cast<const uint2*>(p); return make_uint4(v.x, v.y, 0u, 0u); }
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        return make_uint4(q[0], q[1], 0u, 0u);
    } else {
        const uint8_t* p = blocks + j * 16;
        if (((uintptr_t)p & 15) == 0) return *reinterpret_cast<const uint4*>(p);
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        return make_uint4(q[0], q[1], q[2], q[3]);
    }
}

} // namespace itw
