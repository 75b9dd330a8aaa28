// decode_chain_host_check.cpp -- the host code behind itwDecodeChain, itwDecodeBlocks and itwDdsImage that needs no device, as a stand-alone
// program for a sanitizer run: the format table (csrc/bcn_format.hpp), the argument checks and the descriptor / staging layout
// (csrc/decode_chain_host.hpp) and the DDS payload walk (csrc/dds.hip, host-only, compiled as C++).  Build and run from the repository root:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/decode_chain_host_check.cpp \
//       -x c++ intel-texture-works-plugin_amd/csrc/dds.hip -o /tmp/decode_chain_host_check && /tmp/decode_chain_host_check
// Prints "ok <checks>" and exits 0, or names the first check that failed.  Not covered: everything behind the checks that talks to the
// HIP runtime (pointer kinds, copies, launches) and the kernel itself.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../intel-texture-works-plugin_amd/csrc/decode_chain_host.hpp"
#include "../include/itw_dds.h"

static int g_checks = 0;
#define CHECK(c) do { g_checks++; if (!(c)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main()
{
    using namespace itw;
    const int formats[] = {71, 72, 77, 78, 80, 81, 83, 84, 95, 98, 99};
    std::vector<uint8_t> texels(64 * 64 * 8), blocks(4096);
    uint8_t *p = texels.data(), *b = blocks.data();

    for (int f : formats) {
        const int kind = format_kind(f);
        CHECK(kind != BCN_NONE);
        int seen = 0;
        with_kind(kind, [&](auto K) { seen = K.value; });
        CHECK(seen == kind);
        const int px = texel_bytes(kind);
        CHECK(px == (f == 95 ? 8 : 4));
        CHECK(block_bytes(kind) == (int)itwDdsLevelBytes((uint32_t)f, 4, 4));
        CHECK(keeps_partial_blocks(kind) == (f == 80 || f == 81 || f == 83 || f == 84));
        CHECK(filled_alpha(kind) == (f == 80 || f == 83 ? 255 : f == 81 || f == 84 ? 127 : f == 95 ? 0x3C00 : -1));
        const rgba_surface good{p, 8, 8, 8 * px};
        CHECK(decode_chain_check(kind, b, &good, 1) == 4);
        CHECK(decode_chain_check(kind, b, &good, 0) == 0);
        CHECK(decode_chain_check(kind, nullptr, nullptr, 0) == 0);
        CHECK(decode_chain_check(kind, b, &good, -1) == -1);
        CHECK(decode_chain_check(kind, nullptr, &good, 1) == -1);
        CHECK(decode_chain_check(kind, b, nullptr, 1) == -1);
        const rgba_surface bad[] = {
            {nullptr, 8, 8, 8 * px}, {p, 0, 8, 8 * px}, {p, 8, 0, 8 * px}, {p, -4, 8, 8 * px}, {p, 8, -1, 8 * px}, {p, 8, 8, 8 * px - 4},
            {p, 7, 8, 7 * px + 2}, {p, 32768, 16388, 32768 * px}, {p, 8, 8, -64},
        };
        for (const rgba_surface& s : bad) {
            CHECK(decode_chain_check(kind, b, &s, 1) == -1);
            const rgba_surface two[2] = {good, s};
            CHECK(decode_chain_check(kind, b, two, 2) == -1);
        }
        // the largest image that passes: exactly ITW_MEASURE_MAX_BLOCKS blocks
        const rgba_surface big{p, 32768, 16384, 32768 * px};
        CHECK(decode_chain_check(kind, b, &big, 1) == (int64_t)ITW_MEASURE_MAX_BLOCKS);

        // descriptors and staging layout of a chain with every residue mod 4 and a 70-image tail
        std::vector<rgba_surface> chain = {{p, 37, 21, 37 * px}, {p, 18, 10, 20 * px}, {p, 9, 5, 9 * px}, {p, 4, 2, 4 * px}, {p, 2, 1, 2 * px}, {p, 1, 1, px}};
        for (int i = 0; i < 70; i++) chain.push_back(rgba_surface{p + 4 * i, 1, 1, px});
        const int n = (int)chain.size();
        const int64_t total = decode_chain_check(kind, b, chain.data(), n);
        CHECK(total == 10 * 6 + 5 * 3 + 3 * 2 + 1 + 1 + 1 + 70);
        std::vector<DecodeImage> desc((size_t)n);
        for (int staged = 0; staged < 2; staged++) {
            const DecodeLayout L0 = decode_chain_describe(kind, chain.data(), n, total, nullptr, staged, staged, staged, staged, desc.data());
            std::vector<uint8_t> dev(L0.bytes + 1);
            const DecodeLayout L = decode_chain_describe(kind, chain.data(), n, total, dev.data(), staged, staged, staged, staged, desc.data());
            CHECK(L.bytes == L0.bytes && L.desc == 0 && L.blocks >= (size_t)n * sizeof(DecodeImage));
            int64_t first = 0;
            size_t end = L.texels;
            for (int i = 0; i < n; i++) {
                const DecodeImage& d = desc[(size_t)i];
                CHECK(d.first_block == first && d.width == chain[(size_t)i].width && d.height == chain[(size_t)i].height);
                CHECK(d.blocks_x == (d.width + 3) / 4);
                if (staged) {
                    CHECK(d.ptr == dev.data() + end && (end & 255) == 0 && (d.stride & 15) == 0 && d.stride >= (int64_t)d.width * px);
                    end += decode_chain_up((size_t)d.stride * (size_t)d.height);
                    dev[(size_t)(d.ptr - dev.data()) + (size_t)d.stride * (size_t)d.height - 1] = 1;      // the last staged byte is inside
                } else {
                    CHECK(d.ptr == chain[(size_t)i].ptr && d.stride == chain[(size_t)i].stride);
                }
                first += image_blocks(chain[(size_t)i]);
            }
            CHECK(first == total);
            if (staged) {
                CHECK(end == L.bytes);
                CHECK(L.modes >= L.blocks + (size_t)total * (size_t)block_bytes(kind) && L.min_alpha >= L.modes + (size_t)total * 4);
                CHECK(L.texels >= L.min_alpha + (size_t)n * 4);
            } else {
                CHECK(L.bytes == decode_chain_up((size_t)n * sizeof(DecodeImage)));
            }
        }

        // itwDecodeBlocks' rules: whole blocks unless the format keeps partial ones; a stride that is a multiple of 4, at least the row, an int32
        const bool partial = keeps_partial_blocks(kind);
        CHECK(decode_blocks_check(kind, 8, 8, 8 * px) == 4 && decode_blocks_check(kind, 8, 8, 8 * px + 4) == 4);
        CHECK(decode_blocks_check(kind, 8, 8, 8 * px + 2) == -1 && decode_blocks_check(kind, 8, 8, 8 * px - 4) == -1);
        CHECK(decode_blocks_check(kind, 8, 8, 0) == -1 && decode_blocks_check(kind, 8, 8, -8 * px) == -1);
        CHECK(decode_blocks_check(kind, 8, 8, (int64_t)INT32_MAX - 3) == 4 && decode_blocks_check(kind, 8, 8, (int64_t)INT32_MAX + 1) == -1);
        CHECK(decode_blocks_check(kind, 6, 8, 8 * px) == (partial ? 4 : -1) && decode_blocks_check(kind, 8, 6, 8 * px) == (partial ? 4 : -1));
        CHECK(decode_blocks_check(kind, 5, 7, 8 * px) == (partial ? 4 : -1) && decode_blocks_check(kind, 1, 1, 8 * px) == (partial ? 1 : -1));
        CHECK(decode_blocks_check(kind, 0, 4, 8 * px) == -1 && decode_blocks_check(kind, 4, 0, 8 * px) == -1 && decode_blocks_check(kind, -4, 4, 8 * px) == -1);
        // no ITW_MEASURE_MAX_BLOCKS cap here: the image the chain entry points refuse passes (8193 x 4096 blocks; only the arithmetic runs)
        CHECK(decode_blocks_check(kind, 32772, 16384, 32772 * (int64_t)px) == (int64_t)8193 * 4096);
        // and the bound of one launch, 2^31 - 1 blocks: 46340^2 is the largest square below it
        CHECK(decode_blocks_check(kind, 4 * 46340, 4 * 46340, 4 * 46340 * (int64_t)px) == (int64_t)46340 * 46340);
        CHECK(decode_blocks_check(kind, 4 * 46341, 4 * 46341, 4 * 46341 * (int64_t)px) == -1);
    }
    CHECK(DECODE_IMAGE_MAX_BLOCKS == 0x7fffffff && image_blocks(rgba_surface{nullptr, INT32_MAX, INT32_MAX, 0}) == ((int64_t)1 << 29) * ((int64_t)1 << 29));
    CHECK(format_kind(96) == BCN_BC6H && format_kind(72) == BCN_BC1 && format_kind(78) == BCN_BC3 && format_kind(99) == BCN_BC7);
    CHECK(decode_blocks_check(format_kind(96), 8, 8, 64) == 4);      // itwDecodeBlocks reads BC6H_SF16 as unsigned; the chain entry points refuse it
    const int refused[] = {0, 28, 70, 73, 74, 82, 94, 97, 100, -1};
    for (int f : refused) {
        const rgba_surface good{p, 8, 8, 64};
        CHECK(format_kind(f) == BCN_NONE);
        CHECK(decode_chain_check(format_kind(f), b, &good, 1) == -1);
        CHECK(decode_chain_check(format_kind(f), b, &good, 0) == -1);
        CHECK(decode_blocks_check(format_kind(f), 8, 8, 64) == -1);
        int calls = 0;
        with_kind(format_kind(f), [&](auto) { calls++; });
        CHECK(calls == 0);
    }

    // itwDdsImage: running sums over 2D, mipped, cube and array descriptions
    const uint32_t written[] = {71, 72, 77, 78, 80, 81, 83, 84, 95, 96, 98, 99};
    const uint32_t shapes[][5] = {{37, 21, 1, 0, 1}, {37, 21, 6, 0, 1}, {1023, 517, 10, 0, 1}, {16, 16, 5, 1, 1}, {64, 64, 7, 1, 3}, {5, 9, 4, 0, 4},
                                  {1, 1, 1, 0, 1}, {1, 7, 3, 0, 2}, {16, 16, 5, 1, 0}};
    for (uint32_t f : written)
        for (const auto& s : shapes) {
            const ItwDdsDesc d{s[0], s[1], s[2], f, s[3], s[4]};
            size_t at = itwDdsHeaderBytes(&d);
            CHECK(at == 128 || at == 148);
            uint32_t i = 0;
            for (uint32_t item = 0; item < (s[4] ? s[4] : 1) * (s[3] ? 6u : 1u); item++) {
                uint32_t w = s[0], h = s[1];
                for (uint32_t m = 0; m < s[2]; m++, i++) {
                    uint32_t gw = 0, gh = 0; size_t off = 0;
                    const size_t n = itwDdsImage(&d, i, &gw, &gh, &off);
                    CHECK(n == itwDdsLevelBytes(f, w, h) && gw == w && gh == h && off == at);
                    CHECK(itwDdsImage(&d, i, nullptr, nullptr, nullptr) == n);
                    at += n;
                    w = w > 1 ? w / 2 : 1; h = h > 1 ? h / 2 : 1;
                }
            }
            CHECK(at == itwDdsFileBytes(&d));
            uint32_t gw = 7, gh = 7; size_t off = 7;
            CHECK(itwDdsImage(&d, i, &gw, &gh, &off) == 0 && itwDdsImage(&d, 0xFFFFFFFFu, &gw, &gh, &off) == 0 && gw == 7 && gh == 7 && off == 7);
        }
    const ItwDdsDesc unread{16, 16, 1, 28, 0, 1};
    CHECK(itwDdsImage(nullptr, 0, nullptr, nullptr, nullptr) == 0 && itwDdsImage(&unread, 0, nullptr, nullptr, nullptr) == 0);
    std::printf("ok %d\n", g_checks);
    return 0;
}
