// image_list_host_check.cpp -- the part of the texel stages that needs no device (csrc/image_list_host.hpp: the per-image argument check and
// the staging plan of mipgen.hip, mip_alpha.hip and normal_prep.hip), as a stand-alone program for a sanitizer run.  Build and run from the
// repository root:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/image_list_host_check.cpp -o /tmp/image_list_host_check
//   /tmp/image_list_host_check
// Prints "ok <checks>" and exits 0, or names the first check that failed.  Not covered: the pointer kinds, the copies and everything else
// that talks to the HIP runtime (the strided views in guarded canvases of tests/test_gpu_mipgen.py, test_gpu_alpha_mips.py,
// test_gpu_normal_prep.py and test_gpu_normal_snorm.py).
#include <algorithm>
#include <cstdio>
#include <vector>
#include "../intel-texture-works-plugin_amd/csrc/image_list_host.hpp"

static int g_checks = 0;
#define CHECK(c) do { g_checks++; if (!(c)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

using namespace itw;

struct Size { int w, h; };
static const Size kSizes[] = {{1, 1}, {3, 5}, {4, 4}, {17, 2}, {64, 64}};
alignas(256) static uint8_t g_texels[64 * 64 * 16 + 256];          // never read: the checks and the plan look at addresses only

static rgba_surface tight(Size s, int tb) { return rgba_surface{g_texels, s.w, s.h, s.w * tb}; }

// the rules of a host plan over `im`, and the device form of the same list
static int check_plans(const std::vector<rgba_surface>& im, int tb, size_t head)
{
    const int n = (int)im.size();
    const StagingPlan host(im.data(), n, tb, false, head);
    CHECK((int)host.at.size() == n);
    uint8_t* const bases[2] = {g_texels, g_texels + 256};
    for (int i = 0; i < n; i++) {
        const size_t row = (size_t)im[(size_t)i].width * tb, off = host.at[(size_t)i].offset, pitch = (size_t)host.stride(i);
        CHECK(off % 256 == 0 && off >= head);
        CHECK(pitch % 16 == 0 && pitch >= row && pitch < row + 16 && host.row_bytes(i) == row);
        const size_t end = off + pitch * (size_t)im[(size_t)i].height;
        if (i + 1 < n) CHECK(host.at[(size_t)i + 1].offset >= end && host.at[(size_t)i + 1].offset == up256(end));
        else           CHECK(host.bytes == up256(end));
        for (uint8_t* base : bases) CHECK(host.ptr(i, base) == base + off);      // sized first, bound to a buffer afterwards: the same offsets
    }
    if (n == 0) CHECK(host.bytes == up256(head));
    const StagingPlan dev(im.data(), n, tb, true, head);
    CHECK(dev.at.empty() && dev.bytes == up256(head));
    for (int i = 0; i < n; i++) CHECK(dev.ptr(i, nullptr) == im[(size_t)i].ptr && dev.stride(i) == im[(size_t)i].stride);
    return 0;
}

int main()
{
    // the small sums
    CHECK(up256(0) == 0 && up256(1) == 256 && up256(255) == 256 && up256(256) == 256 && up256(257) == 512);
    const int64_t quads[] = {1, 5, 4, 10, 1024};
    for (int k = 0; k < 5; k++) CHECK(texel_quads(kSizes[k].w, kSizes[k].h) == quads[k]);
    CHECK(quads_fit_one_launch(0) && quads_fit_one_launch((int64_t)0x7fffffff * 256) && !quads_fit_one_launch((int64_t)0x7fffffff * 256 + 1));

    // the per-image check: every fault kind alone, and the first of two
    for (int tb : {4, 8, 16})
        for (const Size sz : kSizes) {
            const rgba_surface good = tight(sz, tb);
            for (int align : {0, tb}) CHECK(image_fault(good, tb, align) == IMAGE_OK);
            rgba_surface s = good; s.ptr = nullptr;
            CHECK(image_fault(s, tb, tb) == IMAGE_NULL_TEXELS);
            s.width = 0;                                            // null texels and no size: the pointer is reported
            CHECK(image_fault(s, tb, tb) == IMAGE_NULL_TEXELS);
            for (int bad : {0, -1, -sz.w}) {
                s = good; s.width = bad;
                CHECK(image_fault(s, tb, tb) == IMAGE_SIZE);
                s = good; s.height = bad;
                CHECK(image_fault(s, tb, tb) == IMAGE_SIZE);
            }
            s = good; s.width = 0; s.stride = -1; s.ptr = g_texels + 1;      // no size, a stride below the row, misaligned: the size is reported
            CHECK(image_fault(s, tb, tb) == IMAGE_SIZE);
            for (int bad : {sz.w * tb - 1, 0, -sz.w * tb}) {
                s = good; s.stride = bad;
                CHECK(image_fault(s, tb, tb) == IMAGE_STRIDE && image_fault(s, tb, 0) == IMAGE_STRIDE);
            }
            s = good; s.stride = sz.w * tb - 1; s.ptr = g_texels + 1;        // a stride below the row, misaligned: the stride is reported
            CHECK(image_fault(s, tb, tb) == IMAGE_STRIDE);
            for (int by : {1, tb / 2, tb - 1}) {
                s = good; s.ptr = g_texels + by;
                CHECK(image_fault(s, tb, tb) == IMAGE_ALIGN);
                CHECK(image_fault(s, tb, 0) == IMAGE_OK);                    // alignment 0 asks for none
                s = good; s.stride = sz.w * tb + by;                         // the row step counts only where there is a second row
                CHECK(image_fault(s, tb, tb) == (sz.h > 1 ? IMAGE_ALIGN : IMAGE_OK));
                CHECK(image_fault(s, tb, 0) == IMAGE_OK);
            }
            s = good; s.stride = sz.w * tb + 16 * tb;                        // row padding of whole texels is no fault
            CHECK(image_fault(s, tb, tb) == IMAGE_OK);

            // in a list: the first faulty image and its kind
            for (const Size other : kSizes) {
                rgba_surface list[3] = {tight(other, tb), good, tight(other, tb)};
                ImageFault f = image_list_fault(list, 3, tb, tb);
                CHECK(!f && f.kind == IMAGE_OK && f.index == -1);
                list[1].stride = sz.w * tb - 1;
                f = image_list_fault(list, 3, tb, tb);
                CHECK(f && f.kind == IMAGE_STRIDE && f.index == 1);
                list[2].ptr = nullptr;                                       // a later fault does not displace it
                f = image_list_fault(list, 3, tb, tb);
                CHECK(f.kind == IMAGE_STRIDE && f.index == 1);
                list[1] = good;
                f = image_list_fault(list, 3, tb, tb);
                CHECK(f.kind == IMAGE_NULL_TEXELS && f.index == 2);
                CHECK(!image_list_fault(list, 2, tb, tb) && !image_list_fault(list, 0, tb, tb));
            }
        }

    // the staging plan: single images, every pair, the whole list both ways round, padded rows, the empty list
    for (int tb : {4, 8, 16})
        for (size_t head : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257}) {
            std::vector<rgba_surface> all;
            for (const Size a : kSizes) {
                all.push_back(tight(a, tb));
                if (check_plans({tight(a, tb)}, tb, head)) return 1;
                for (const Size b : kSizes) {
                    rgba_surface padded = tight(b, tb);
                    padded.ptr += tb; padded.stride += 3 * tb;               // a view: the plan's pitch is the row's, not the caller's
                    if (check_plans({tight(a, tb), padded}, tb, head)) return 1;
                }
            }
            if (check_plans(all, tb, head)) return 1;
            std::reverse(all.begin(), all.end());
            if (check_plans(all, tb, head)) return 1;
            if (check_plans({}, tb, head)) return 1;
        }

    // against the sums the stages made inline before there was a plan (generate_chain: a 16-byte table entry per image, then the coverage
    // passes' work, then the images): the full chains of two 130 x 66 items
    {
        const int items = 2, levels = 8, count = items * levels;
        for (int px : {4, 8})
            for (size_t work : {(size_t)0, (size_t)4096 + 256}) {
                std::vector<rgba_surface> im;
                for (int i = 0; i < count; i++) {
                    const int l = i % levels, w = std::max(1, 130 >> l), h = std::max(1, 66 >> l);
                    im.push_back(rgba_surface{g_texels + 4 * px, w, h, w * px + 2 * px});
                }
                CHECK(im[7].width == 1 && im[7].height == 1 && im[1].width == 65 && im[1].height == 33);
                auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
                size_t bytes = up((size_t)count * 16);
                bytes += work;
                std::vector<size_t> stage_off((size_t)count), stride((size_t)count);
                for (int i = 0; i < count; i++) {
                    stride[(size_t)i] = ((size_t)im[(size_t)i].width * px + 15) & ~(size_t)15;
                    stage_off[(size_t)i] = bytes;
                    bytes += up(stride[(size_t)i] * (size_t)im[(size_t)i].height);
                }
                const StagingPlan plan(im.data(), count, px, false, up256((size_t)count * 16) + work);
                for (int i = 0; i < count; i++)
                    CHECK(plan.at[(size_t)i].offset == stage_off[(size_t)i] && (size_t)plan.stride(i) == stride[(size_t)i]);
                CHECK(plan.bytes == bytes);
            }
    }
    std::printf("ok %d\n", g_checks);
    return 0;
}
