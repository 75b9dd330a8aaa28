// host_runs.hpp -- the part of a host-pointer encode call (abi.hip compress()) that needs no device: into which runs of block rows the call
// is cut, and where each run's slice of the per-thread workspace lies when the runs are bands.  Plain C++, no HIP headers, no getenv: a
// host-only program checks it under a sanitizer (tools/host_runs_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include "bcn_format.hpp"

namespace itw {

constexpr int kMaxHostRuns = 8;

// Run c covers block rows [cut[c], cut[c + 1]) of the surface; n runs, cut[0] = 0, cut[n] = by.
struct HostRuns {
    int n = 1;
    int cut[kMaxHostRuns + 1] = {0};
    int rows(int c) const { return (cut[c + 1] - cut[c]) * 4; }      // texel rows of run c (the formats that are cut keep no partial blocks)
};

// BC7 / BC6H spend milliseconds per surface: the call is cut into runs of block rows so that the upload of run c+1 and the download of run
// c-1 (copy stream; a pageable copy blocks only this host thread) overlap the kernels of run c.  A run must still fill the chip several
// times over (one block per lane: 1024 workgroups = one round of the BC7 scans), or the kernels' tails cost more than the copies save --
// measured at 4096^2 (tools/history/misc/host_chunks_probe.py): BC7 slow 9.58 / 9.19 / 9.60 / 11.6 ms for 1 / 2 / 4 / 8 runs, BC6H slow
// 7.61 / 6.15 / 5.64 / 5.57 ms.  BC1/3/4/5 are PCIe-bound: one run.  Runs need not be equal: a SHORT FIRST run starts the kernels after an
// eighth of the upload instead of half of it, and a shorter last run shortens the download nothing can hide.
// In order of precedence, the later rule replacing the earlier: the default split of a large BC7 / BC6H call; `chunks` (ITW_HOST_CHUNKS: 1 .. 8
// equal runs where by >= 4 * v; 1 disables the overlap); `runs` (ITW_HOST_RUNS: up to 7 cumulative fractions "0.125,0.625" -> 3 runs, where
// by >= 64; every run keeps at least one block row).  A device source is never cut.  The knobs' values come as strings, null when unset.
inline HostRuns host_runs(int kind, int bx, int by, bool src_host, const char* chunks, const char* runs)
{
    HostRuns r;
    int* cut = r.cut;
    cut[1] = by;
    if (!src_host) return r;
    if (kind == BCN_BC7 && (int64_t)bx * by >= 524288)       { r.n = 3; cut[1] = by / 8; cut[2] = by / 8 + by / 2; cut[3] = by; }
    else if (kind == BCN_BC6H && (int64_t)bx * by >= 262144) { r.n = 4; cut[1] = by / 8; cut[2] = by * 3 / 8; cut[3] = by * 11 / 16; cut[4] = by; }
    if (chunks) {
        const int v = std::atoi(chunks);
        if (v >= 1 && v <= kMaxHostRuns && by >= 4 * v) { r.n = v; for (int c = 0; c <= v; c++) cut[c] = (int)((int64_t)by * c / v); }
    }
    if (runs) {
        int n = 0; double f[kMaxHostRuns];
        for (const char* p = runs; *p && n < kMaxHostRuns - 1;) { char* q = nullptr; f[n] = std::strtod(p, &q); if (q == p) break; n++; p = (*q == ',') ? q + 1 : q; }
        if (n > 0 && by >= 64) {
            r.n = n + 1; cut[0] = 0; cut[r.n] = by;
            for (int c = 0; c < n; c++) { int t = (int)(by * f[c]); cut[c + 1] = t < cut[c] + 1 ? cut[c] + 1 : (t > by - (n - c) ? by - (n - c) : t); }
        }
    }
    return r;
}

// The most workspace any one run needs, `bytes(rows)` being the need of a run of `rows` texel rows.  "Most demanding" is not "tallest"
// (ADVICE r02): a staged BC7 run of up to 2^20 blocks takes the wide shape at ~440 B/block while a taller one takes the deep shape at
// 36 B/block, so the maximum is taken over every run's own need.
template <class Bytes>
inline size_t host_runs_workspace(const HostRuns& r, Bytes&& bytes)
{
    size_t need = 0;
    for (int c = 0; c < r.n; c++)
        if (r.rows(c) > 0) { const size_t b = bytes(r.rows(c)); if (b > need) need = b; }
    return need;
}

// The workspace of a BC7 call whose runs are bands: [wide runs (they follow each other on one stream)] [probe] [band 0] [band 1] ..., each
// piece rounded to 256 bytes.  `bytes(rows, wide)`: what a run of `rows` texel rows needs as a wide run (`wide`) or as a band; the probe
// is a band over the first run's rows.
struct BandWorkspace { size_t probe_off = 0, band_off[kMaxHostRuns] = {0}, total = 0; };
template <class Bytes>
inline BandWorkspace band_workspace(const HostRuns& r, Bytes&& bytes)
{
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    BandWorkspace L;
    L.probe_off = up(host_runs_workspace(r, [&](int rows) { return bytes(rows, true); }));
    L.total = L.probe_off + up(bytes(r.rows(0), false));
    for (int c = 0; c < r.n; c++) {
        L.band_off[c] = L.total;
        if (r.rows(c) > 0) L.total += up(bytes(r.rows(c), false));
    }
    return L;
}

} // namespace itw
