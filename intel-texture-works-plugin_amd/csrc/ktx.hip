// ktx.hip -- KTX 1.1 container for ETC1 block streams (the itwKtx* part of include/itw_dds.h); host code only.
// Layout: Khronos KTX File Format Specification 1.1, sections 2 (header) and 3 (fields).  Data order: for each mip level its imageSize
// word, then the level's faces; ETC1 images are multiples of 8 bytes, so cubePadding and mipPadding are always empty.
#include <cstring>
#include "../../include/itw_dds.h"

namespace {

constexpr uint8_t KTX_ID[12] = {0xAB, 0x4B, 0x54, 0x58, 0x20, 0x31, 0x31, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A};
constexpr uint32_t KTX_ENDIAN = 0x04030201u, GL_ETC1_RGB8_OES = 0x8D64u, GL_RGB = 0x1907u;
constexpr size_t KTX_HEADER = 64;
constexpr uint32_t KTX_MAX_LEVELS = 32;                   // a full chain from 2^31 texels

void put32(uint8_t* p, size_t word, uint32_t v) { std::memcpy(p + 12 + 4 * word, &v, 4); }      // word w of the 13 behind the identifier
uint32_t get32(const uint8_t* p, size_t byte) { uint32_t v; std::memcpy(&v, p + byte, 4); return v; }

bool valid(const ItwKtxDesc* d)
{
    return d && d->gl_internal_format == GL_ETC1_RGB8_OES && d->width && d->height && d->mip_levels >= 1 && d->mip_levels <= KTX_MAX_LEVELS &&
           (!d->is_cubemap || d->width == d->height);
}
uint32_t faces(const ItwKtxDesc& d) { return d.is_cubemap ? 6u : 1u; }
uint64_t image_bytes(uint32_t w, uint32_t h) { return (((uint64_t)w + 3) / 4) * (((uint64_t)h + 3) / 4) * 8u; }
uint32_t next(uint32_t v) { return v > 1 ? v / 2 : 1; }

} // namespace

extern "C" {

size_t itwKtxHeaderBytes(const ItwKtxDesc* d) { return valid(d) ? KTX_HEADER : 0; }

size_t itwKtxFileBytes(const ItwKtxDesc* d)
{
    if (!valid(d)) return 0;
    uint64_t total = KTX_HEADER + d->key_value_bytes;
    uint32_t w = d->width, h = d->height;
    for (uint32_t l = 0; l < d->mip_levels; l++) {
        total += 4 + image_bytes(w, h) * faces(*d);
        w = next(w); h = next(h);
    }
    return (size_t)total;
}

size_t itwKtxWriteHeader(const ItwKtxDesc* d, uint8_t* dst, size_t capacity)
{
    if (!valid(d) || d->key_value_bytes != 0 || !dst || capacity < KTX_HEADER) return 0;
    std::memcpy(dst, KTX_ID, 12);
    put32(dst, 0, KTX_ENDIAN);
    put32(dst, 1, 0);                                       // glType: compressed
    put32(dst, 2, 1);                                       // glTypeSize
    put32(dst, 3, 0);                                       // glFormat: compressed
    put32(dst, 4, GL_ETC1_RGB8_OES);
    put32(dst, 5, GL_RGB);
    put32(dst, 6, d->width);
    put32(dst, 7, d->height);
    put32(dst, 8, 0);                                       // pixelDepth: 2D
    put32(dst, 9, 0);                                       // numberOfArrayElements: no array
    put32(dst, 10, faces(*d));
    put32(dst, 11, d->mip_levels);
    put32(dst, 12, 0);                                      // bytesOfKeyValueData
    return KTX_HEADER;
}

size_t itwKtxReadHeader(const uint8_t* src, size_t size, ItwKtxDesc* out)
{
    if (!src || !out || size < KTX_HEADER || std::memcmp(src, KTX_ID, 12) != 0) return 0;
    if (get32(src, 12) != KTX_ENDIAN) return 0;             // the other byte order reads as 0x01020304
    ItwKtxDesc d;
    d.gl_internal_format = get32(src, 28);
    d.width = get32(src, 36); d.height = get32(src, 40);
    const uint32_t depth = get32(src, 44), elements = get32(src, 48), nfaces = get32(src, 52);
    d.mip_levels = get32(src, 56) ? get32(src, 56) : 1;
    d.key_value_bytes = get32(src, 60);
    if (depth != 0 || elements != 0 || (nfaces != 1 && nfaces != 6)) return 0;
    d.is_cubemap = nfaces == 6 ? 1 : 0;
    if (!valid(&d)) return 0;
    const uint64_t total = (uint64_t)KTX_HEADER + d.key_value_bytes;      // where the levels begin
    if (total > size || itwKtxFileBytes(&d) > size) return 0;
    // every level's size word against the sizes
    uint64_t pos = total;
    uint32_t w = d.width, h = d.height;
    for (uint32_t l = 0; l < d.mip_levels; l++) {
        const uint64_t n = image_bytes(w, h);
        if (get32(src, (size_t)pos) != n) return 0;         // one face of a cube, the level otherwise (one image either way: no arrays)
        pos += 4 + n * nfaces;
        w = next(w); h = next(h);
    }
    *out = d;
    return (size_t)total;
}

size_t itwKtxImage(const ItwKtxDesc* d, uint32_t index, uint32_t* width, uint32_t* height, size_t* offset)
{
    if (!valid(d)) return 0;
    const uint32_t nf = faces(*d);
    if ((uint64_t)index >= (uint64_t)nf * d->mip_levels) return 0;
    const uint32_t level = index / nf, face = index - level * nf;
    uint64_t pos = (uint64_t)KTX_HEADER + d->key_value_bytes;
    uint32_t w = d->width, h = d->height;
    for (uint32_t l = 0; l < level; l++) {
        pos += 4 + image_bytes(w, h) * nf;
        w = next(w); h = next(h);
    }
    const uint64_t n = image_bytes(w, h);
    if (width) *width = w;
    if (height) *height = h;
    if (offset) *offset = (size_t)(pos + 4 + n * face);
    return (size_t)n;
}

size_t itwKtxWriteFile(const ItwKtxDesc* d, const uint8_t* const* levels, size_t nlevels, uint8_t* dst, size_t capacity)
{
    const size_t total = itwKtxFileBytes(d);
    if (!total || d->key_value_bytes != 0 || !levels || !dst || capacity < total) return 0;
    const uint32_t nf = faces(*d);
    if (nlevels != (size_t)nf * d->mip_levels) return 0;
    size_t pos = itwKtxWriteHeader(d, dst, capacity);
    if (!pos) return 0;
    size_t idx = 0;
    uint32_t w = d->width, h = d->height;
    for (uint32_t l = 0; l < d->mip_levels; l++) {
        const size_t n = (size_t)image_bytes(w, h);
        const uint32_t word = (uint32_t)n;
        if ((uint64_t)word != (uint64_t)n) return 0;        // an image of 4 GiB or more has no size word
        std::memcpy(dst + pos, &word, 4);
        pos += 4;
        for (uint32_t f = 0; f < nf; f++) {
            if (!levels[idx]) return 0;
            std::memcpy(dst + pos, levels[idx], n);
            pos += n; idx++;
        }
        w = next(w); h = next(h);
    }
    return pos;
}

} // extern "C"
