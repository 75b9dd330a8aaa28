// dds.hip -- DDS container for BCn block streams (include/itw_dds.h); host code only.
// Header contents follow DirectXTex's _EncodeDDSHeader for the formats the plugin saves
// (DirectXTexDDS.cpp:441-675; constants DDS.h:38-236); data order as SaveToDDSMemory (:1611-1700):
// for each array item / cube face, its mip chain from the top level down, tightly packed.
#include <cstring>
#include "../../include/itw_dds.h"

namespace {

constexpr uint32_t DDS_MAGIC = 0x20534444;                 // "DDS "
constexpr uint32_t DDS_FOURCC = 0x4;
constexpr uint32_t HEADER_FLAGS_TEXTURE = 0x00001007, HEADER_FLAGS_MIPMAP = 0x00020000, HEADER_FLAGS_LINEARSIZE = 0x00080000;
constexpr uint32_t SURFACE_FLAGS_TEXTURE = 0x00001000, SURFACE_FLAGS_MIPMAP = 0x00400008, SURFACE_FLAGS_CUBEMAP = 0x00000008;
constexpr uint32_t CUBEMAP_ALLFACES = 0x0000fe00;
constexpr uint32_t DIMENSION_TEXTURE2D = 3, MISC_TEXTURECUBE = 0x4;
constexpr uint32_t HEADER_FLAGS_VOLUME = 0x00800000, CAPS2_VOLUME = 0x00200000, DIMENSION_TEXTURE3D = 4;     // DDS.h: DDS_HEADER_FLAGS_VOLUME, DDS_FLAGS_VOLUME

constexpr uint32_t fourcc(char a, char b, char c, char d)
{
    return (uint32_t)(uint8_t)a | ((uint32_t)(uint8_t)b << 8) | ((uint32_t)(uint8_t)c << 16) | ((uint32_t)(uint8_t)d << 24);
}

// the two BC1A codes (itw_dispatch.h) are stored as what their streams are: BC1, 71 / 72; the two BC2 codes as DXGI's BC2, 74 / 75; the two
// BC3_DXTEX codes as what their streams are: BC3, 77 / 78
uint32_t stored_format(uint32_t f)
{
    return f == 0x83F1u ? 71u : f == 0x8C4Du ? 72u : f == 0x83F2u ? 74u : f == 0x8C4Eu ? 75u : f == 0x83F3u ? 77u : f == 0x8C4Fu ? 78u : f;
}
// what itwDdsReadHeader reports for a file's own code: BC2 goes by its two codes in a descriptor as everywhere else (74 / 75 as descriptor codes stay refused)
uint32_t descriptor_format(uint32_t stored) { return stored == 74u ? 0x83F2u : stored == 75u ? 0x8C4Eu : stored; }

int bytes_per_block(uint32_t f)
{
    if (f == 74u || f == 75u) return 0;                     // a descriptor says ITW_FORMAT_BC2_UNORM[_SRGB]
    switch (stored_format(f)) {
    case 71: case 72: case 80: case 81: return 8;           // BC1, BC4_UNORM, BC4_SNORM
    case 74: case 75:                                       // BC2
    case 77: case 78: case 83: case 84: case 95: case 96: case 98: case 99: return 16;   // BC3, BC5_UNORM, BC5_SNORM, BC6H, BC7
    default: return 0;
    }
}

// legacy FourCC for the formats DirectXTex maps without the DX10 extension
// (DirectXTexDDS.cpp:474-483; DDS.h:71-96: BC4_UNORM -> "BC4U", BC4_SNORM -> "BC4S", BC5_UNORM -> "BC5U", BC5_SNORM -> "BC5S")
uint32_t legacy_fourcc(uint32_t f)
{
    switch (stored_format(f)) {
    case 71: return fourcc('D', 'X', 'T', '1');
    case 74: return fourcc('D', 'X', 'T', '3');
    case 77: return fourcc('D', 'X', 'T', '5');
    case 80: return fourcc('B', 'C', '4', 'U');
    case 81: return fourcc('B', 'C', '4', 'S');
    case 83: return fourcc('B', 'C', '5', 'U');
    case 84: return fourcc('B', 'C', '5', 'S');
    default: return 0u;
    }
}

bool needs_dx10(const ItwDdsDesc& d)
{
    // arrays other than a single cube need the extension (DirectXTexDDS.cpp:450-457)
    const uint32_t items = d.array_size ? d.array_size : 1;
    return legacy_fourcc(d.dxgi_format) == 0 || (items > 1 && d.is_cubemap != 2);      // (2: ITW_DDS_VOLUME, whose array_size is a depth; a volume is never an array)
}

// the format a legacy FourCC names, 0 for none
uint32_t legacy_format(uint32_t cc)
{
    if (cc == fourcc('D', 'X', 'T', '1')) return 71;
    if (cc == fourcc('D', 'X', 'T', '3') || cc == fourcc('D', 'X', 'T', '2')) return 74;   // DirectXTexDDS.cpp:58-62: the premultiplied
    if (cc == fourcc('D', 'X', 'T', '5') || cc == fourcc('D', 'X', 'T', '4')) return 77;   // spellings DXT2 / DXT4 read as BC2 / BC3
    if (cc == fourcc('B', 'C', '4', 'U') || cc == fourcc('A', 'T', 'I', '1')) return 80;   // DirectXTexDDS.cpp:64-70
    if (cc == fourcc('B', 'C', '5', 'U') || cc == fourcc('A', 'T', 'I', '2')) return 83;
    if (cc == fourcc('B', 'C', '4', 'S')) return 81;                                         // (the ATI spellings are UNORM only)
    if (cc == fourcc('B', 'C', '5', 'S')) return 84;
    return 0;
}

// a volume (ITW_DDS_VOLUME in is_cubemap; array_size is its depth): _EncodeDDSHeader's TEX_DIMENSION_TEXTURE3D case
// (DirectXTexDDS.cpp:585-597), payload level-major (:1167-1200)
bool is_volume(const ItwDdsDesc& d) { return d.is_cubemap == ITW_DDS_VOLUME; }
uint32_t half_of(uint32_t v) { return v > 1 ? v / 2 : 1; }

void put32(uint8_t* p, size_t word, uint32_t v) { std::memcpy(p + 4 * word, &v, 4); }
uint32_t get32(const uint8_t* p, size_t word) { uint32_t v; std::memcpy(&v, p + 4 * word, 4); return v; }

} // namespace

extern "C" {

size_t itwDdsLevelBytes(uint32_t f, uint32_t w, uint32_t h)
{
    const size_t nbw = (w + 3) / 4 ? (w + 3) / 4 : 1, nbh = (h + 3) / 4 ? (h + 3) / 4 : 1;
    return nbw * nbh * (size_t)bytes_per_block(f);
}

size_t itwDdsHeaderBytes(const ItwDdsDesc* d)
{
    if (!d || !bytes_per_block(d->dxgi_format) || !d->width || !d->height || !d->mip_levels) return 0;
    if (is_volume(*d) && !d->array_size) return 0;                       // a depth of 0
    return 4 + 124 + (needs_dx10(*d) ? 20 : 0);
}

size_t itwDdsFileBytes(const ItwDdsDesc* d)
{
    const size_t hdr = itwDdsHeaderBytes(d);
    if (!hdr) return 0;
    size_t chain = 0;
    uint32_t w = d->width, h = d->height, z = is_volume(*d) ? d->array_size : 1;
    for (uint32_t m = 0; m < d->mip_levels; m++) {
        chain += itwDdsLevelBytes(d->dxgi_format, w, h) * (size_t)z;
        w = half_of(w); h = half_of(h); z = half_of(z);
    }
    if (is_volume(*d)) return hdr + chain;
    const size_t items = (size_t)(d->array_size ? d->array_size : 1) * (d->is_cubemap ? 6 : 1);
    return hdr + chain * items;
}

size_t itwDdsWriteHeader(const ItwDdsDesc* d, uint8_t* dst, size_t capacity)
{
    const size_t need = itwDdsHeaderBytes(d);
    if (!need || !dst || capacity < need) return 0;
    std::memset(dst, 0, need);
    put32(dst, 0, DDS_MAGIC);
    uint8_t* h = dst + 4;                                   // DDS_HEADER, 31 dwords
    put32(h, 0, 124);                                       // dwSize
    put32(h, 1, HEADER_FLAGS_TEXTURE | HEADER_FLAGS_MIPMAP | HEADER_FLAGS_LINEARSIZE | (is_volume(*d) ? HEADER_FLAGS_VOLUME : 0u));   // mipLevels > 0 always sets MIPMAP (:553); volume :593
    put32(h, 2, d->height);
    put32(h, 3, d->width);
    put32(h, 4, (uint32_t)itwDdsLevelBytes(d->dxgi_format, d->width, d->height));         // slice pitch of the top level
    put32(h, 5, is_volume(*d) ? d->array_size : 1);         // dwDepth = 1 for 2D (:576), the depth of a volume (:597)
    put32(h, 6, d->mip_levels);
    uint32_t caps = SURFACE_FLAGS_TEXTURE, caps2 = 0;
    if (d->mip_levels > 1) caps |= SURFACE_FLAGS_MIPMAP;
    if (is_volume(*d)) caps2 |= CAPS2_VOLUME;               // :594
    else if (d->is_cubemap) { caps |= SURFACE_FLAGS_CUBEMAP; caps2 |= CUBEMAP_ALLFACES; }
    // ddspf at dwords 18..25
    put32(h, 18, 32);
    put32(h, 19, DDS_FOURCC);
    put32(h, 20, needs_dx10(*d) ? fourcc('D', 'X', '1', '0') : legacy_fourcc(d->dxgi_format));
    put32(h, 26, caps);
    put32(h, 27, caps2);
    if (needs_dx10(*d)) {
        uint8_t* e = h + 124;                               // DDS_HEADER_DXT10
        put32(e, 0, stored_format(d->dxgi_format));
        put32(e, 1, is_volume(*d) ? DIMENSION_TEXTURE3D : DIMENSION_TEXTURE2D);
        put32(e, 2, d->is_cubemap && !is_volume(*d) ? MISC_TEXTURECUBE : 0);
        put32(e, 3, is_volume(*d) ? 1 : d->array_size ? d->array_size : 1);     // cubes: number of cubes (:646-650); a volume: 1
        put32(e, 4, 0);                                     // miscFlags2 stays 0 unless forced (:664-668)
    }
    return need;
}

size_t itwDdsReadHeader(const uint8_t* src, size_t size, ItwDdsDesc* out)
{
    if (!src || !out || size < 128 || get32(src, 0) != DDS_MAGIC) return 0;
    const uint8_t* h = src + 4;
    if (get32(h, 0) != 124 || get32(h, 18) != 32 || !(get32(h, 19) & DDS_FOURCC)) return 0;
    const bool volume = (get32(h, 1) & HEADER_FLAGS_VOLUME) != 0;        // DirectXTex's test for "volume", either header kind (DirectXTexDDS.cpp:291, :323-328)
    ItwDdsDesc d;
    d.height = get32(h, 2); d.width = get32(h, 3);
    d.mip_levels = get32(h, 6) ? get32(h, 6) : 1;
    d.is_cubemap = (get32(h, 27) & 0x200) ? 1 : 0;
    d.array_size = 1;
    size_t off = 128;
    const uint32_t cc = get32(h, 20);
    if ((d.dxgi_format = legacy_format(cc)) != 0) {}
    else if (cc == fourcc('D', 'X', '1', '0')) {
        if (size < 148) return 0;
        const uint8_t* e = h + 124;
        d.dxgi_format = get32(e, 0);
        if (get32(e, 1) != (volume ? DIMENSION_TEXTURE3D : DIMENSION_TEXTURE2D)) return 0;
        if (volume && get32(e, 3) > 1) return 0;            // a volume is no array (:294-296)
        d.is_cubemap = (get32(e, 2) & MISC_TEXTURECUBE) ? 1 : 0;
        d.array_size = get32(e, 3) ? get32(e, 3) : 1;
        off = 148;
    } else return 0;
    if (d.dxgi_format == 0x83F2u || d.dxgi_format == 0x8C4Eu || d.dxgi_format == 0x83F3u || d.dxgi_format == 0x8C4Fu) return 0;          // (no file holds the library's own codes)
    d.dxgi_format = descriptor_format(d.dxgi_format);
    if (!bytes_per_block(d.dxgi_format) || !d.width || !d.height) return 0;
    if (volume) {                                           // the payload is level-major: the depth travels in array_size
        if (!get32(h, 5)) return 0;
        d.is_cubemap = ITW_DDS_VOLUME;
        d.array_size = get32(h, 5);
    }
    *out = d;
    return off;
}

size_t itwDdsImage(const ItwDdsDesc* d, uint32_t index, uint32_t* width, uint32_t* height, size_t* offset)
{
    const size_t hdr = itwDdsHeaderBytes(d);
    if (!hdr) return 0;
    if (is_volume(*d)) {                                    // level-major: the slices of level 0, then those of level 1, ...
        size_t pos = hdr;
        uint64_t first = 0;
        uint32_t w = d->width, h = d->height, z = d->array_size;
        for (uint32_t m = 0; m < d->mip_levels; m++) {
            const size_t n = itwDdsLevelBytes(d->dxgi_format, w, h);
            if ((uint64_t)index < first + z) {
                if (width) *width = w;
                if (height) *height = h;
                if (offset) *offset = pos + (size_t)(index - first) * n;
                return n;
            }
            first += z; pos += n * (size_t)z;
            w = half_of(w); h = half_of(h); z = half_of(z);
        }
        return 0;
    }
    const uint64_t items = (uint64_t)(d->array_size ? d->array_size : 1) * (d->is_cubemap ? 6 : 1);
    if ((uint64_t)index >= items * d->mip_levels) return 0;
    const uint32_t item = index / d->mip_levels, mip = index - item * d->mip_levels;
    size_t chain = 0, before = 0, bytes = 0;
    uint32_t w = d->width, h = d->height;
    for (uint32_t m = 0; m < d->mip_levels; m++) {
        const size_t n = itwDdsLevelBytes(d->dxgi_format, w, h);
        if (m == mip) { before = chain; bytes = n; if (width) *width = w; if (height) *height = h; }
        chain += n;
        w = w > 1 ? w / 2 : 1; h = h > 1 ? h / 2 : 1;
    }
    if (offset) *offset = hdr + (size_t)item * chain + before;
    return bytes;
}

size_t itwDdsWriteFile(const ItwDdsDesc* d, const uint8_t* const* levels, size_t nlevels, uint8_t* dst, size_t capacity)
{
    const size_t total = itwDdsFileBytes(d);
    if (!total || !levels || !dst || capacity < total) return 0;
    if (is_volume(*d)) {                                    // `levels` are the slices in file order; the images follow each other without gaps
        size_t at = itwDdsWriteHeader(d, dst, capacity);
        if (!at) return 0;
        for (size_t i = 0; ; i++) {
            const size_t n = i <= 0xffffffffu ? itwDdsImage(d, (uint32_t)i, nullptr, nullptr, nullptr) : 0;
            if (!n) return i == nlevels ? at : 0;
            if (i >= nlevels || !levels[i]) return 0;
            std::memcpy(dst + at, levels[i], n);
            at += n;
        }
    }
    const size_t items = (size_t)(d->array_size ? d->array_size : 1) * (d->is_cubemap ? 6 : 1);
    if (nlevels != items * d->mip_levels) return 0;
    size_t pos = itwDdsWriteHeader(d, dst, capacity);
    if (!pos) return 0;
    size_t idx = 0;
    for (size_t it = 0; it < items; it++) {
        uint32_t w = d->width, h = d->height;
        for (uint32_t m = 0; m < d->mip_levels; m++) {
            const size_t n = itwDdsLevelBytes(d->dxgi_format, w, h);
            if (!levels[idx]) return 0;
            std::memcpy(dst + pos, levels[idx], n);
            pos += n; idx++;
            w = w > 1 ? w / 2 : 1; h = h > 1 ? h / 2 : 1;
        }
    }
    return pos;
}

} // extern "C"
