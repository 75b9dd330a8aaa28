// offset32_host_check.cpp -- the rule that lets the BC1 / BC3 / BC4 / BC5 kernels walk a surface with 32-bit byte offsets
// (csrc/offset32_host.hpp walk_fits_32), checked against the walk itself without a device, as a stand-alone program for a sanitizer run.
// Build and run from the repository root:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/offset32_host_check.cpp -o /tmp/offset32_host_check
//   /tmp/offset32_host_check
// Prints "ok <checks>" and exits 0, or names the first check that failed.
// For a few thousand (stride, width, height) triples -- rows that overlap, widths up to 2^31 - 1, the two strides around the switch -- it
// replays what a lane of bc13_kernel<SMALL> / bc45_kernel<WHOLE> computes: the first offset, off_step, off_wrap, the clamp to the last block
// and the four row addresses, once in uint32_t as the kernel does and once in int64_t, and asserts
//   - both give the same addresses wherever the rule says "32-bit",
//   - the rule says "32-bit" for every surface of non-overlapping rows with height * stride < 2^31 (the route those surfaces always took),
//   - the rule it replaces (height * stride < 2^31 alone, bc4_bc5.hip's before) does wrap on a surface of overlapping rows, which the rule refuses.
// Not covered: the kernels themselves (tests/test_gpu_large_offsets.py runs both routes on either side of the switch), and a block count
// beyond int32, which neither route of the BC4 / BC5 launcher handles (the replay skips such triples).
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include "../intel-texture-works-plugin_amd/csrc/offset32_host.hpp"

static long g_checks = 0;
#define CHECK(c) do { g_checks++; if (!(c)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

using itw::walk_fits_32;

struct Walk {
    int64_t stride;
    int width, height;      // texels
    int bw;                 // bytes of a block's row: 16 (RGBA8), 32 (RGBA16F), 64 (RGBA32F)
    int lanes;              // lanes per block: 1 (BC1, BC3, BC4), 2 (BC5)
    int64_t grid;           // workgroups of 256 lanes
};

// 0: every address of the sampled lanes agrees; else the line of the first disagreement.  The caller has made sure that the lane count fits
// an int32, as the kernels' arguments need.
static int replay(const Walk& k, long* visited)
{
    const int32_t blocks_x = k.width / 4, blocks_y = k.height / 4;
    const int64_t nblocks = (int64_t)blocks_x * blocks_y;
    const int32_t per_wg = 256 / k.lanes;                                  // blocks of one workgroup's chunk
    const int64_t step_blocks64 = k.grid * per_wg;
    const int32_t step_blocks = (int32_t)step_blocks64;
    const int32_t step_y = step_blocks / blocks_x, step_x = step_blocks - step_y * blocks_x;
    const uint32_t stride32 = (uint32_t)k.stride, BW = (uint32_t)k.bw;
    const uint32_t off_step = (uint32_t)step_y * 4u * stride32 + (uint32_t)step_x * BW;
    const uint32_t off_wrap = 4u * stride32 - (uint32_t)blocks_x * BW;
    const int64_t off_step64 = (int64_t)step_y * 4 * k.stride + (int64_t)step_x * k.bw;
    const int64_t off_wrap64 = 4 * k.stride - (int64_t)blocks_x * k.bw;
    // the clamp, as each kernel writes it (the same block for a surface of whole blocks)
    const int32_t ly = (int32_t)((nblocks - 1) / blocks_x);
    const uint32_t last13 = (uint32_t)ly * 4u * stride32 + (uint32_t)(nblocks - 1 - (int64_t)ly * blocks_x) * 16u;
    const uint32_t last45 = (uint32_t)(k.height / 4 - 1) * 4u * stride32 + (uint32_t)(blocks_x - 1) * BW;
    const int64_t last64 = (int64_t)(blocks_y - 1) * 4 * k.stride + (int64_t)(blocks_x - 1) * k.bw;
    if ((k.bw == 16 && (int64_t)last13 != last64) || (int64_t)last45 != last64) return __LINE__;
    for (int y = 0; y < 4; y++)
        if ((int64_t)(uint32_t)(last45 + (uint32_t)y * stride32) != last64 + y * k.stride) return __LINE__;
    const int64_t wgs[3] = {0, k.grid / 2, k.grid - 1};
    const int32_t slots[3] = {0, per_wg / 2 + 1, per_wg - 1};              // a lane's block within its workgroup's chunk
    for (int64_t wg : wgs)
        for (int32_t slot : slots) {
            int64_t cur = wg * per_wg + slot;
            if (cur >= nblocks) continue;                                  // such a lane starts on the clamp, checked above
            const int32_t yy = (int32_t)(cur / blocks_x);
            int32_t xx = (int32_t)(cur - (int64_t)yy * blocks_x);
            uint32_t off = (uint32_t)yy * 4u * stride32 + (uint32_t)xx * BW;
            int64_t off64 = (int64_t)yy * 4 * k.stride + (int64_t)xx * k.bw;
            for (;;) {
                const int64_t by = cur / blocks_x, bx = cur - by * blocks_x;
                const int64_t direct = by * 4 * k.stride + bx * k.bw;      // the 64-bit loaders' address of the same block
                if (off64 != direct || (int64_t)off != off64 || xx != (int32_t)bx) return __LINE__;
                for (int y = 0; y < 4; y++)
                    if ((int64_t)(uint32_t)(off + (uint32_t)y * stride32) != off64 + y * k.stride) return __LINE__;
                ++*visited;
                cur += step_blocks64;
                if (cur >= nblocks) break;
                xx += step_x; off += off_step; off64 += off_step64;
                if (xx >= blocks_x) { xx -= blocks_x; off += off_wrap; off64 += off_wrap64; }
            }
        }
    return 0;
}

// the grids the launchers use: bc13_grid's bound for BC1 / BC3, BC45_GRID for the others
static int64_t grid_of(int64_t nlanes, bool bc13)
{
    const int64_t chunks = (nlanes + 255) / 256;
    const int64_t bound = bc13 ? (chunks <= 8192 ? 3072 : 6144) : 2048;
    return chunks < bound ? chunks : bound;
}

static bool old_whole(int64_t stride, int height) { return stride > 0 && stride < ((int64_t)1 << 31) && (int64_t)height * stride < ((int64_t)1 << 31); }

static long g_walked = 0, g_visited = 0, g_refused = 0;

// one triple through every launcher's form of the rule
static int check_triple(int64_t stride, int width, int height)
{
    struct Form { int bw, lanes, out_per_block; bool bc13; };
    static const Form forms[] = {{16, 1, 8, true}, {16, 1, 16, true}, {16, 1, 0, false}, {16, 2, 0, false}, {32, 2, 0, false}, {64, 2, 0, false}};
    for (const Form& f : forms) {
        const int64_t nblocks = (int64_t)(width / 4) * (height / 4);
        const bool fits = walk_fits_32(stride, width, height, f.bw, nblocks * f.out_per_block);
        const int64_t row_bytes = (int64_t)(width / 4) * f.bw;
        if (nblocks > 0 && stride >= row_bytes && old_whole(stride, height)) CHECK(fits);      // the route these surfaces always took
        if (!old_whole(stride, height)) CHECK(!fits);                                           // and nothing new walks
        if (!fits) { g_refused++; continue; }
        CHECK(nblocks > 0 && stride > 0);
        if (nblocks * f.lanes > 0x7fffffff) continue;
        const Walk k{stride, width, height, f.bw, f.lanes, grid_of(nblocks * f.lanes, f.bc13)};
        CHECK(replay(k, &g_visited) == 0);
        g_walked++;
    }
    return 0;
}

int main()
{
    const int64_t G2 = (int64_t)1 << 31;
    // the switch: eight rows at 2^28 - 16 and at 2^28 bytes apart are 2^31 - 128 and 2^31 bytes
    for (int bw : {16, 32, 64}) {
        CHECK(walk_fits_32(((int64_t)1 << 28) - 16, 1028, 8, bw, 0));
        CHECK(!walk_fits_32((int64_t)1 << 28, 1028, 8, bw, 0));
    }
    CHECK(walk_fits_32(4 * 16384, 16384, 16384, 16, (int64_t)4096 * 4096 * 16));              // 16384^2 RGBA8, 1 GiB
    CHECK(walk_fits_32(4 * 16384, 16384, 32764, 16, 0) && !walk_fits_32(4 * 16384, 16384, 32768, 16, 0));
    CHECK(!walk_fits_32(0, 64, 64, 16, 0) && !walk_fits_32(-256, 64, 64, 16, 0));             // the walk needs rows that ascend
    CHECK(!walk_fits_32(256, 64, 64, 16, (int64_t)1 << 32) && walk_fits_32(256, 64, 64, 16, ((int64_t)1 << 32) - 8));

    // the hole: rows 16 bytes apart, 2^28 + 1 blocks wide.  height * stride is 64, and the last block's row starts 2^32 bytes in
    {
        const Walk hole{16, (1 << 30) + 4, 4, 16, 1, grid_of((1 << 28) + 1, false)};
        long seen = 0;
        CHECK(old_whole(hole.stride, hole.height));
        CHECK(replay(hole, &seen) != 0);                                                      // the 32-bit walk misplaces it
        for (int bw : {16, 32, 64}) CHECK(!walk_fits_32(hole.stride, hole.width, hole.height, bw, 0));
        const Walk below{16, (1 << 29) - 16, 4, 16, 1, grid_of((1 << 27) - 4, false)};       // the widest such surface the rule lets walk
        CHECK(walk_fits_32(below.stride, below.width, below.height, 16, 0) && replay(below, &seen) == 0);
        CHECK(!walk_fits_32(16, (1 << 29) - 12, 4, 16, 0));
    }

    static const int heights[] = {3, 4, 7, 8, 12, 16, 60, 64, 1024, 4100, 16384, 32768, 1 << 20, 0x7fffffff};
    static const int widths[] = {3, 4, 8, 1028, 4096, 16384, 65540, 1 << 20, (1 << 24) + 4, (1 << 28) - 4, 1 << 28, (1 << 29) - 8, 1 << 29, (1 << 30) + 4,
                                 0x7ffffffc, 0x7fffffff};
    for (int h : heights)
        for (int w : widths) {
            const int64_t tight = (int64_t)w * 4;
            const int64_t strides[] = {4, 16, 48, 4096, tight / 2 & ~(int64_t)3, tight - 16, tight, tight + 4, tight + 16, 2 * tight, 4 * tight, 16 * tight,
                                       ((int64_t)1 << 28) - 16, (int64_t)1 << 28, 0x30000000, (G2 - 1) / h & ~(int64_t)15, ((G2 - 1) / h & ~(int64_t)15) + 16,
                                       G2 / h, G2 / h - 4, G2 - 16, G2, 2 * G2, -tight, 0};
            for (int64_t s : strides) if (check_triple(s, w, h)) return 1;
        }
    // and triples from a fixed sequence: sizes and strides of every magnitude, overlapping rows as often as not
    uint64_t r = 0x9e3779b97f4a7c15ull;
    auto next = [&r]() { r ^= r << 13; r ^= r >> 7; r ^= r << 17; return r; };
    for (int i = 0; i < 4000; i++) {
        const int w = (int)(next() >> (33 + next() % 28)) + 1, h = (int)(next() >> (33 + next() % 28)) + 1;
        int64_t s = (int64_t)(next() >> (32 + next() % 30)) + 1;
        if (i & 1) s = (int64_t)w * 4 + (int64_t)(s & 0xfff0);                                  // rows that do not overlap
        if (check_triple(s & ~(int64_t)3, w, h)) return 1;
    }
    CHECK(g_walked > 2000 && g_refused > 2000 && g_visited > 100000);
    std::printf("ok %ld checks, %ld walks replayed over %ld blocks, %ld refused\n", g_checks, g_walked, g_visited, g_refused);
    return 0;
}
