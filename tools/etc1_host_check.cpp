// etc1_host_check.cpp -- the ETC1 encoder's arithmetic (csrc/etc1_core.hpp: the text the kernel of csrc/etc1.hip is built from) run on the
// host, one lane after the other, against the reference's own CompressBlocksETC1 from oracle/_ref/libispc_texcomp_ref_full.so.  It checks the
// reading of the reference -- division sites, clamps, tie-breaks, bit packing -- without a GPU; what it cannot check is the kernel's cross-lane
// selection and reductions.  Build and run from the repository root (after build() has made oracle/_ref):
//   g++ -std=c++17 -O2 -ffp-contract=off -Iinclude -Ioracle tools/etc1_host_check.cpp -ldl -o /tmp/etc1_host_check
//   /tmp/etc1_host_check oracle/_ref/libispc_texcomp_ref_full.so [blocks per side of each test surface: default 32 = 14 336 blocks in all]
// tests/test_etc1_cpu.py builds it and runs it with 16 blocks per side (3 584 blocks).
// (add -g -fsanitize=address,undefined -fno-sanitize-recover=all for a sanitizer run of the same text: it is host code with its own main)
// Prints the blocks compared per threshold and "ok", or the first block that differs.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <vector>
extern "C" {
#include "x86_math.h"
}
#include "../include/ispc_texcomp.h"
#include "../intel-texture-works-plugin_amd/csrc/etc1_core.hpp"

using namespace itw::etc1;

struct HalfFit { float err; int table; uint32_t qbits; int qc[3]; };

static HalfFit fit_half(const Half& h, const Sorted& s, const std::vector<int32_t>& keys, int flip, int half, bool diff, const int (&prev)[3],
                        int threshold, const float* inv)
{
    HalfFit best{255.f * 255.f * 3.f * 8.f, -1, 0u, {0, 0, 0}};
    for (int i = 0; i < threshold; i++)
        for (int table = 0; table < 8; table++) {
            uint32_t qbits;
            int qc[3];
            const float dy[4] = {(float)modifier(table, 0), (float)modifier(table, 1), (float)modifier(table, 2), (float)modifier(table, 3)};
            const float err = eval_candidate(h, s.rank, flip, half, keys[(size_t)i] & 0xFFF, dy, diff, prev, inv, qbits, qc);
            if (err < best.err) best = HalfFit{err, table, qbits, {qc[0], qc[1], qc[2]}};
        }
    return best;
}

static void encode_block(const uint8_t* src, int stride, int threshold, const float* inv, uint32_t (&out)[2])
{
    const SplitTable splits = make_split_table();
    float best_err = 1.0f / 0.0f;
    for (int flip = 0; flip < 2; flip++) {
        Half h[2];
        Sorted s[2];
        std::vector<int32_t> keys[2];
        for (int half = 0; half < 2; half++) {
            for (int kk = 0; kk < 8; kk++) {
                const uint8_t* t = src + texel_row(flip, half, kk) * stride + texel_col(flip, half, kk) * 4;
                for (int p = 0; p < 3; p++) h[half].px[p][kk] = (float)t[p];
            }
            sort_half(h[half], s[half]);
            for (int i = 0; i < SPLITS; i++) keys[half].push_back(split_key(s[half].y, splits.v[i], inv));
            std::sort(keys[half].begin(), keys[half].end());
        }
        for (int diff = 1; diff >= 0; diff--) {
            const int none[3] = {-1, -1, -1};
            const HalfFit a = fit_half(h[0], s[0], keys[0], flip, 0, diff, none, threshold, inv);
            const HalfFit b = fit_half(h[1], s[1], keys[1], flip, 1, diff, a.qc, threshold, inv);
            float err = 0.f;
            err += a.err;
            err += b.err;
            if (err < best_err) {
                best_err = err;
                const int qc[2][3] = {{a.qc[0], a.qc[1], a.qc[2]}, {b.qc[0], b.qc[1], b.qc[2]}};
                const int table[2] = {a.table, b.table};
                pack_block(qc, table, a.qbits | b.qbits, diff, flip, out);
            }
        }
    }
}

typedef void (*RefEncode)(const rgba_surface*, uint8_t*, etc_enc_settings*);

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s <libispc_texcomp_ref_full.so> [blocks per side, default 32]\n", argv[0]); return 2; }
    const int side = argc > 2 ? std::atoi(argv[2]) : 32;
    if (side < 1 || side > 64) { std::fprintf(stderr, "blocks per side: 1 .. 64\n"); return 2; }
    void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!lib) { std::fprintf(stderr, "%s\n", dlerror()); return 2; }
    RefEncode ref = (RefEncode)dlsym(lib, "CompressBlocksETC1");
    if (!ref) { std::fprintf(stderr, "no CompressBlocksETC1 in %s\n", argv[1]); return 2; }

    float inv[9] = {0.f};
    for (int n = 1; n <= 8; n++) inv[n] = ispc_rcp((float)n);

    // side x side blocks: noise, a noisy ramp per block, few colours, smooth
    const int W = 4 * side, H = 4 * side;
    uint32_t rng = 12345u;
    auto next = [&] { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
    std::vector<uint8_t> img((size_t)W * H * 4);
    for (int kind = 0; kind < 4; kind++) {
        for (int by = 0; by < H / 4; by++)
            for (int bx = 0; bx < W / 4; bx++) {
                const int base[3] = {(int)(next() & 255), (int)(next() & 255), (int)(next() & 255)};
                const int other[3] = {(int)(next() & 255), (int)(next() & 255), (int)(next() & 255)};
                const int amp = 1 + bx * 127 / (side > 1 ? side - 1 : 1);
                for (int y = 0; y < 4; y++)
                    for (int x = 0; x < 4; x++) {
                        uint8_t* t = &img[((size_t)(by * 4 + y) * W + bx * 4 + x) * 4];
                        const bool pick = next() & 1;
                        for (int p = 0; p < 3; p++) {
                            int v;
                            if (kind == 0) v = (int)(next() & 255);
                            else if (kind == 1) v = base[p] + (int)(next() % (2 * amp + 1)) - amp;
                            else if (kind == 2) v = pick ? base[p] : other[p];
                            else v = ((bx * 4 + x) * (p + 1) + (by * 4 + y) * (3 - p)) / 2 + (int)(next() & 3);
                            t[p] = (uint8_t)std::min(255, std::max(0, v));
                        }
                        t[3] = (uint8_t)next();
                    }
            }
        for (int threshold : {1, 2, 6, 32}) {
            if (threshold == 32 && kind > 1) continue;
            rgba_surface surf{img.data(), W, H, W * 4};
            etc_enc_settings st{threshold};
            std::vector<uint8_t> want((size_t)(W / 4) * (H / 4) * 8);
            ref(&surf, want.data(), &st);
            int bad = 0;
            for (int by = 0; by < H / 4; by++)
                for (int bx = 0; bx < W / 4; bx++) {
                    uint32_t got[2];
                    encode_block(&img[((size_t)by * 4 * W + bx * 4) * 4], W * 4, threshold, inv, got);
                    const uint8_t* w = &want[((size_t)by * (W / 4) + bx) * 8];
                    if (std::memcmp(got, w, 8) != 0 && bad++ == 0)
                        std::fprintf(stderr, "surface %d threshold %d block (%d, %d): got %08x %08x, reference %02x%02x%02x%02x %02x%02x%02x%02x (bytes)\n", kind,
                                     threshold, bx, by, got[0], got[1], w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]);
                }
            std::printf("surface %d threshold %d: %d of %d blocks differ\n", kind, threshold, bad, (W / 4) * (H / 4));
            if (bad) return 1;
        }
    }
    std::printf("ok\n");
    return 0;
}
