// host_runs_check.cpp -- the part of a host-pointer encode call that needs no device (csrc/host_runs.hpp: the run cuts and the band workspace
// layout of abi.hip's compress()), as a stand-alone program for a sanitizer run.  Build and run from the repository root:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/host_runs_check.cpp -o /tmp/host_runs_check \
//       && /tmp/host_runs_check
// Prints "ok <checks>" and exits 0, or names the first check that failed.  Not covered: which streams the runs go to and everything else
// that talks to the HIP runtime (tests/test_gpu_host_runs_small.py, tests/test_gpu_host_pointer_runs.py).
#include <cstdio>
#include <initializer_list>
#include "../intel-texture-works-plugin_amd/csrc/host_runs.hpp"

static int g_checks = 0;
#define CHECK(c) do { g_checks++; if (!(c)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static bool cuts_are(const itw::HostRuns& r, std::initializer_list<int> want)
{
    if (r.n != (int)want.size() - 1) return false;
    int c = 0;
    for (int v : want) if (r.cut[c++] != v) return false;
    return true;
}

int main()
{
    using namespace itw;
    const char* none = nullptr;
    // the default splits and their thresholds
    CHECK(cuts_are(host_runs(BCN_BC7, 1024, 512, true, none, none), {0, 64, 320, 512}));
    CHECK(cuts_are(host_runs(BCN_BC7, 1024, 511, true, none, none), {0, 511}));
    CHECK(cuts_are(host_runs(BCN_BC6H, 512, 512, true, none, none), {0, 64, 192, 352, 512}));
    CHECK(cuts_are(host_runs(BCN_BC6H, 512, 511, true, none, none), {0, 511}));
    CHECK(cuts_are(host_runs(BCN_BC7, 512, 512, true, none, none), {0, 512}));            // (BC6H's threshold is not BC7's)
    for (int kind : {BCN_BC1, BCN_BC3, BCN_BC4, BCN_BC5, BCN_BC4S, BCN_BC5S, BCN_ETC1})
        for (int by : {1, 63, 512, 16384}) CHECK(cuts_are(host_runs(kind, 16384, by, true, none, none), {0, by}));
    // ITW_HOST_CHUNKS: 1 .. 8 equal runs where by >= 4 * v, for every format
    for (int kind : {BCN_BC7, BCN_BC1}) {
        CHECK(cuts_are(host_runs(kind, 16, 130, true, "4", none), {0, 32, 65, 97, 130}));
        CHECK(cuts_are(host_runs(kind, 16, 131, true, "4", none), {0, 32, 65, 98, 131}));
        CHECK(cuts_are(host_runs(kind, 16, 16, true, "4", none), {0, 4, 8, 12, 16}));
        CHECK(cuts_are(host_runs(kind, 16, 15, true, "4", none), {0, 15}));
        CHECK(cuts_are(host_runs(kind, 16, 130, true, "0", none), {0, 130}));
        CHECK(cuts_are(host_runs(kind, 16, 130, true, "9", none), {0, 130}));
        CHECK(cuts_are(host_runs(kind, 16, 130, true, "-1", none), {0, 130}));
        CHECK(cuts_are(host_runs(kind, 16, 130, true, "x", none), {0, 130}));
        CHECK(cuts_are(host_runs(kind, 16, 64, true, "8", none), {0, 8, 16, 24, 32, 40, 48, 56, 64}));
    }
    CHECK(cuts_are(host_runs(BCN_BC7, 1024, 512, true, "1", none), {0, 512}));             // 1 takes the default split away
    CHECK(cuts_are(host_runs(BCN_BC7, 1024, 512, true, "9", none), {0, 64, 320, 512}));    // an ignored value leaves it
    // ITW_HOST_RUNS: up to 7 cumulative fractions where by >= 64, every run at least one block row
    CHECK(cuts_are(host_runs(BCN_BC7, 16, 64, true, none, "0.125,0.625"), {0, 8, 40, 64}));
    CHECK(cuts_are(host_runs(BCN_BC7, 16, 64, true, none, "0.9,0.1"), {0, 57, 58, 64}));
    CHECK(cuts_are(host_runs(BCN_BC7, 16, 64, true, none, "0,0,0"), {0, 1, 2, 3, 64}));
    CHECK(cuts_are(host_runs(BCN_BC7, 16, 64, true, none, "1.5"), {0, 63, 64}));
    CHECK(cuts_are(host_runs(BCN_BC7, 16, 64, true, none, "-3"), {0, 1, 64}));
    CHECK(cuts_are(host_runs(BCN_BC7, 16, 64, true, none, "0.125,0.25,0.375,0.5,0.625,0.75,0.875,0.9375"), {0, 8, 16, 24, 32, 40, 48, 56, 64}));
    CHECK(cuts_are(host_runs(BCN_BC7, 16, 64, true, none, "1,1,1,1,1,1,1,1"), {0, 57, 58, 59, 60, 61, 62, 63, 64}));
    CHECK(cuts_are(host_runs(BCN_BC7, 16, 64, true, none, "0.5,x"), {0, 32, 64}));         // the parse stops at what is no number
    CHECK(cuts_are(host_runs(BCN_BC7, 16, 64, true, none, ""), {0, 64}));
    CHECK(cuts_are(host_runs(BCN_BC7, 16, 63, true, none, "0.125,0.625"), {0, 63}));
    CHECK(cuts_are(host_runs(BCN_BC1, 16, 64, true, none, "0.5"), {0, 32, 64}));
    CHECK(cuts_are(host_runs(BCN_BC7, 1024, 512, true, none, "0.5"), {0, 256, 512}));      // replaces the default split
    CHECK(cuts_are(host_runs(BCN_BC7, 16, 64, true, "4", "0.125,0.625"), {0, 8, 40, 64})); // both knobs: the fractions win
    CHECK(cuts_are(host_runs(BCN_BC7, 16, 63, true, "4", "0.125,0.625"), {0, 15, 31, 47, 63}));   // ... where they apply
    // a device source is never cut
    CHECK(cuts_are(host_runs(BCN_BC7, 1024, 512, false, none, none), {0, 512}));
    CHECK(cuts_are(host_runs(BCN_BC6H, 512, 512, false, "4", "0.5"), {0, 512}));
    CHECK(cuts_are(host_runs(BCN_BC1, 16, 64, false, "8", "0.125,0.625"), {0, 64}));
    // whatever the rule: cut[0] = 0, cut[n] = by, ascending, and rows() is four texel rows per block row
    for (int by : {64, 65, 100, 511, 512, 4096})
        for (const char* runs : {none, "0.125,0.625", "0,0,0", "2,2,2,2,2,2,2", "0.3"})
            for (const char* chunks : {none, "1", "3", "8"}) {
                const HostRuns r = host_runs(BCN_BC7, 1024, by, true, chunks, runs);
                CHECK(r.n >= 1 && r.n <= kMaxHostRuns && r.cut[0] == 0 && r.cut[r.n] == by);
                int rows = 0;
                for (int c = 0; c < r.n; c++) { CHECK(r.cut[c + 1] >= r.cut[c]); CHECK(r.rows(c) == 4 * (r.cut[c + 1] - r.cut[c])); rows += r.rows(c); }
                CHECK(rows == 4 * by);
            }

    // the band workspace: [largest wide need] [probe] [band 0] [band 1] ..., every piece a multiple of 256 and none overlapping another
    auto fake = [](int rows, bool wide) { return (size_t)(wide ? (rows <= 256 ? 440 * rows + 7 : 36 * rows + 1) : 100 * rows + 13); };
    for (const char* runs : {"0.125,0.625", "0,0,0", "0.9,0.1", "0.5", "0.1,0.2,0.3,0.4,0.5,0.6,0.7"}) {
        const HostRuns r = host_runs(BCN_BC7, 16, 64, true, none, runs);
        const BandWorkspace L = band_workspace(r, fake);
        size_t widest = 0;
        for (int c = 0; c < r.n; c++) if (fake(r.rows(c), true) > widest) widest = fake(r.rows(c), true);
        CHECK(widest == host_runs_workspace(r, [&](int rows) { return fake(rows, true); }));
        CHECK(L.probe_off == ((widest + 255) & ~(size_t)255) && L.probe_off >= widest);     // the wide runs' piece starts at 0 and ends here
        size_t at = L.probe_off + ((fake(r.rows(0), false) + 255) & ~(size_t)255);          // the probe: a band over the first run's rows
        for (int c = 0; c < r.n; c++) {
            CHECK(L.band_off[c] == at && (at & 255) == 0);
            at += (fake(r.rows(c), false) + 255) & ~(size_t)255;
            CHECK(L.band_off[c] + fake(r.rows(c), false) <= at);
        }
        CHECK(L.total == at);
    }
    {   // "most demanding" is not "tallest": the short run in the wide shape outweighs the tall one in the deep shape
        const HostRuns r = host_runs(BCN_BC7, 16, 512, true, none, "0.125");
        CHECK(r.rows(0) == 256 && r.rows(1) == 1792 && band_workspace(r, fake).probe_off == ((440 * 256 + 7 + 255) & ~(size_t)255));
    }
    {   // a run without rows (a surface a few block rows high and very wide) takes no band slice, and the layout still holds
        const HostRuns r = host_runs(BCN_BC7, 131072, 4, true, none, none);
        CHECK(cuts_are(r, {0, 0, 2, 4}));
        const BandWorkspace L = band_workspace(r, fake);
        CHECK(L.band_off[0] == L.band_off[1] && L.band_off[2] > L.band_off[1] && L.total > L.band_off[2]);
    }
    std::printf("ok %d\n", g_checks);
    return 0;
}
