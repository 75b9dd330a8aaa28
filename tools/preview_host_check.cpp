// preview_host_check.cpp -- the host code behind itwPreviewBlocks / itwPreviewSurface that needs no device (csrc/preview_host.hpp: the argument
// checks, the channel table, the coordinate rule and the row range a host source is uploaded by), as a stand-alone program for a sanitizer
// run.  Build and run from the repository root:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/preview_host_check.cpp \
//       -o /tmp/preview_host_check && /tmp/preview_host_check
// Prints "ok <checks>" and exits 0, or names the first check that failed.  Not covered: everything that talks to the HIP runtime and the kernel.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "../intel-texture-works-plugin_amd/csrc/preview_host.hpp"

static int g_checks = 0;
#define CHECK(c) do { g_checks++; if (!(c)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main()
{
    using namespace itw;
    std::vector<uint8_t> bytes(4096);
    uint8_t* p = bytes.data();
    itw_preview_view v{8, 8, 0, 0, 1.0, 0, 0, 1.0f, 0};
    CHECK(preview_view_ok(&v, sizeof v, p, 24));
    CHECK(!preview_view_ok(&v, sizeof v, p, 23) && !preview_view_ok(&v, sizeof v - 1, p, 24) && !preview_view_ok(nullptr, sizeof v, p, 24) &&
          !preview_view_ok(&v, sizeof v, nullptr, 24));
    for (double z : {0.0, -0.0, -1.0, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()}) {
        itw_preview_view bad = v;
        bad.zoom = z;
        CHECK(!preview_view_ok(&bad, sizeof bad, p, 24));
    }
    for (int32_t off : {(1 << 30) + 1, -(1 << 30) - 1, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()}) {
        itw_preview_view bad = v;
        bad.x_offset = off;
        CHECK(!preview_view_ok(&bad, sizeof bad, p, 24));
        bad = v;
        bad.y_offset = off;
        CHECK(!preview_view_ok(&bad, sizeof bad, p, 24));
    }
    for (int32_t n : {0, -1, 16385}) {
        itw_preview_view bad = v;
        bad.width = n;
        CHECK(!preview_view_ok(&bad, sizeof bad, p, 3 * 16385));
        bad = v;
        bad.height = n;
        CHECK(!preview_view_ok(&bad, sizeof bad, p, 24));
    }
    for (int f : {71, 72, 77, 78, 80, 83, 95, 98, 99, (int)ITW_FORMAT_ETC1_RGB8}) CHECK(preview_blocks_kind(f, p, 37, 21) == format_kind(f));
    for (int f : {81, 84, 96, 0, 74, -1}) CHECK(preview_blocks_kind(f, p, 8, 8) == BCN_NONE);
    CHECK(preview_blocks_kind(98, nullptr, 8, 8) == BCN_NONE && preview_blocks_kind(98, p, 0, 8) == BCN_NONE && preview_blocks_kind(98, p, 32768, 16388) == BCN_NONE);
    const rgba_surface s8{p, 8, 8, 32}, short_row{p, 8, 8, 31}, huge{p, 32768, 16388, 32768 * 4};
    CHECK(preview_surface_ok(&s8, 4) && !preview_surface_ok(&s8, 8) && !preview_surface_ok(&s8, 3) && !preview_surface_ok(&short_row, 4) &&
          !preview_surface_ok(&huge, 4) && !preview_surface_ok(nullptr, 4));

    // the channel table, IntelPlugin.cpp:585-624 with four planes
    const int R = ITW_PREVIEW_CHANNEL_RED, G = ITW_PREVIEW_CHANNEL_GREEN, B = ITW_PREVIEW_CHANNEL_BLUE, A = ITW_PREVIEW_CHANNEL_ALPHA, X = PREVIEW_NO_CHANNEL;
    const struct { int m, c0, c1, c2; bool alone; } table[] = {
        {0, 0, 1, 2, false}, {R, 0, 0, 0, false}, {G, 1, 1, 1, false}, {B, 2, 2, 2, false}, {A, 3, 3, 3, true}, {R | G, 0, 1, X, false},
        {R | B, 0, X, 2, false}, {G | B, X, 1, 2, false}, {R | G | B, 0, 1, 2, false}, {R | A, 0, X, 3, false}, {G | A, X, 1, 3, false},
        {B | A, X, X, 3, false}, {R | G | A, 0, 1, 3, false}, {R | B | A, 0, X, 3, false}, {G | B | A, X, 1, 3, false}, {R | G | B | A, 0, 1, 3, false}};
    for (const auto& t : table) {
        int ch[3]; bool alone;
        preview_channels((uint32_t)t.m | 0xFFFFFFC3u, ch, &alone);
        CHECK(ch[0] == t.c0 && ch[1] == t.c1 && ch[2] == t.c2 && alone == t.alone);
    }

    // coordinates: the fraction rule, the far offsets, and the range against every pixel of it
    int x = -7;
    CHECK(preview_coord(2, -3, 0.5, 10, &x) && x == 0);          // fx = -0.5
    CHECK(!preview_coord(1, -3, 0.5, 10, &x));                   // fx = -1.0
    CHECK(!preview_coord(23, -3, 0.5, 10, &x));                  // fx = W
    CHECK(preview_coord(22, -3, 0.5, 10, &x) && x == 9);
    CHECK(!preview_coord(0, 1 << 30, 1000.0, 16384, &x) && !preview_coord(16383, -(1 << 30), 1e300, 16384, &x));
    CHECK(!preview_coord(5, 1 << 30, std::numeric_limits<double>::max(), 16384, &x));      // the product is +inf
    for (double zoom : {0.125, 1.0 / 3.0, 0.5, 1.0, 1.5, 2.0, 3.7, 16.0, 1000.0})
        for (int off : {-50, -1, 0, 17, 400})
            for (int n : {1, 37, 131}) {
                int lo = 0, hi = 0, seen_lo = 1 << 30, seen_hi = -1;
                const bool any = preview_range(0, 96, off, zoom, n, &lo, &hi);
                for (int t = 0; t <= 96; t++)
                    if (preview_coord(t, off, zoom, n, &x)) { seen_lo = x < seen_lo ? x : seen_lo; seen_hi = x > seen_hi ? x : seen_hi; }
                CHECK(seen_hi < 0 || (any && 0 <= lo && lo <= seen_lo && seen_hi <= hi && hi < n));
            }
    CHECK(preview_span_blocks(PREVIEW_TILE_W, 2.0) == 33 && preview_span_blocks(PREVIEW_TILE_H, 2.0) == 9 && preview_span_blocks(64, 1.0) == 17 &&
          preview_span_blocks(64, 0.25) == 5);
    std::printf("ok %d\n", g_checks);
    return 0;
}
