"""What the cubic and triangle mip filters cost (ITW_MIP_CUBIC / ITW_MIP_TRIANGLE; include/itw_dispatch.h "Mip chains: cubic and triangle";
csrc/mip_filters.hip), in the method of tools/mipgen_timing.py: a call = the entry point followed by a synchronise of the stream, inside a
host clock (time.perf_counter); the legs of a row alternate call by call in one run, so that whatever the clocks do they do to all of them;
per leg the median of reps x inner calls (default 7 x 5 = 35), the fastest call, p10 and p90 -- the run's own spread.  Run it twice.

Rows (one JSON object per line; stdout, and appended to profiles/mip_filter_timing.jsonl unless --no-save), device-resident full chains:
  2d_4096_rgba8 / _rgba16f, cube_1024_rgba8 / _rgba16f   `per_level` (the box filter under ITW_MIP_PER_LEVEL, the route beside which the
           filters are read), `pyramid` (flags 0), `cubic_global` and `cubic_lds` (the cubic filter's two kernels, through the hooks build's
           itwTestMipCubicVariant), `triangle`
  2d_4000x3000_rgba16f                                    `per_level` is the linear filter (flags 0), then the same filter legs
Every leg also as a multiple of the row's per_level median, and as a share of 8 TB/s over `bytes_per_level`: every level but the last read
once and every level but the base written once, what the per-level route moves.
--parent-lib=PATH adds `parent_pyramid` / `parent_per_level` / `parent_cubic` / `parent_triangle` legs to every row: the flags-0,
ITW_MIP_PER_LEVEL, ITW_MIP_CUBIC and ITW_MIP_TRIANGLE calls through another build of libispc_texcomp.so (the parent commit's, whose
cubic kernel is its default's, the one `cubic_global` runs), alternating with this build's in the same run.
Usage: python tools/mip_filter_timing.py [reps] [inner] [--label=TEXT] [--no-save] [--out=PATH] [--only=SUBSTRING] [--parent-lib=PATH]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
import numpy as np                      # noqa: E402
import itw_amd                          # noqa: E402

PEAK_BYTES_PER_US = 8.0e6               # 8 TB/s


def opt(name, default):
    return next((a[len(name) + 3:] for a in sys.argv if a.startswith("--" + name + "=")), default)


def content(h, w, half, seed):
    rng = np.random.default_rng(seed)
    if half:
        return rng.random((h, w, 4), dtype=np.float32).astype(np.float16).view(np.int16)
    return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)


def measure(legs, reps, inner, stream):
    for _ in range(3):                                            # warm-up: code objects, the thread's buffers, clocks
        for _, call in legs:
            call()
    stream.synchronize()
    times = {name: [] for name, _ in legs}
    for _ in range(reps):
        for _ in range(inner):
            for name, call in legs:                               # the legs alternate
                t0 = time.perf_counter()
                call()
                stream.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e6)
    out = {}
    for name, t in times.items():
        t = np.sort(np.array(t))
        out[name] = {"median_us": round(float(np.median(t)), 2), "min_us": round(float(t[0]), 2),
                     "p10_us": round(float(np.percentile(t, 10)), 2), "p90_us": round(float(np.percentile(t, 90)), 2)}
    return out


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    inner = int(args[1]) if len(args) > 1 else 5
    only = opt("only", "")
    out_path = opt("out", os.path.join(ROOT, "profiles", "mip_filter_timing.jsonl"))
    T = itw_amd.test_lib()              # the product's sources with the hooks: every leg of this build runs through one library
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    T.itwSetStream(stream.cuda_stream)
    parent = None
    if opt("parent-lib", ""):
        parent = C.CDLL(os.path.abspath(opt("parent-lib", "")))
        parent.itwSetStream.argtypes = [C.c_void_p]
        parent.itwSetStream.restype = None
        parent.itwGenerateMipChain.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32]
        parent.itwGenerateMipChain.restype = C.c_int
        parent.itwSetStream(stream.cuda_stream)

    def emit(row):
        row.update({"reps": reps, "inner": inner, "calls_per_leg": reps * inner, "label": opt("label", ""), "device": itw_amd.device_info(),
                    "unit": "us per call, host clock around the call + stream synchronise"})
        print(json.dumps(row), flush=True)
        if "--no-save" not in sys.argv:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "a") as f:
                f.write(json.dumps(row) + "\n")

    def device_chains(w, h, items, half):
        n = itw_amd.mip_levels(w, h)
        chains = []
        for i in range(items):
            base = torch.from_numpy(content(h, w, half, 10 + i)).to(dev)
            chains.append([base] + [torch.empty((max(1, h >> l), max(1, w >> l), 4), dtype=base.dtype, device=dev) for l in range(1, n)])
        return chains, n

    def checked(lib, arr, items, n, px, flags, lds=None):
        def call():
            if lds is not None:
                T.itwTestMipCubicVariant(lds)
            if lib.itwGenerateMipChain(arr, items, n, px, flags) != 0:
                raise RuntimeError("itwGenerateMipChain failed: " + (itw_amd.last_error() or ""))
        return call

    for name, w, h, items, half in (("2d_4096_rgba8", 4096, 4096, 1, False), ("2d_4096_rgba16f", 4096, 4096, 1, True),
                                    ("2d_4000x3000_rgba16f", 4000, 3000, 1, True),
                                    ("cube_1024_rgba8", 1024, 1024, 6, False), ("cube_1024_rgba16f", 1024, 1024, 6, True)):
        if only not in name:
            continue
        chains, n = device_chains(w, h, items, half)
        px = 8 if half else 4
        arr = C.cast(itw_amd.abi._surfaces([lv for ch in chains for lv in ch]), C.c_void_p)
        sizes = [max(1, w >> l) * max(1, h >> l) * px for l in range(n)]
        traffic = items * sum(sizes[l - 1] + sizes[l] for l in range(1, n))
        box = (w & (w - 1)) == 0 and (h & (h - 1)) == 0
        legs = [("per_level", checked(T, arr, items, n, px, itw_amd.MIP_PER_LEVEL if box else 0))]
        if box:
            legs.append(("pyramid", checked(T, arr, items, n, px, 0)))
        legs += [("cubic_global", checked(T, arr, items, n, px, itw_amd.MIP_CUBIC, lds=0)), ("cubic_lds", checked(T, arr, items, n, px, itw_amd.MIP_CUBIC, lds=1)),
                 ("triangle", checked(T, arr, items, n, px, itw_amd.MIP_TRIANGLE))]
        if parent is not None:
            legs.append(("parent_per_level", checked(parent, arr, items, n, px, itw_amd.MIP_PER_LEVEL if box else 0)))
            if box:
                legs.append(("parent_pyramid", checked(parent, arr, items, n, px, 0)))
            legs += [("parent_cubic", checked(parent, arr, items, n, px, itw_amd.MIP_CUBIC)), ("parent_triangle", checked(parent, arr, items, n, px, itw_amd.MIP_TRIANGLE))]
        row = {"row": name, "width": w, "height": h, "items": items, "levels": n, "pixel_size": px, "bytes_per_level": traffic,
               "per_level_filter": "box" if box else "linear"}
        try:
            row.update(measure(legs, reps, inner, stream))
        finally:
            T.itwTestMipCubicVariant(0)
        for leg, _ in legs:
            row[leg + "_over_per_level"] = round(row[leg]["median_us"] / row["per_level"]["median_us"], 3)
            row[leg + "_fraction_of_8TBs"] = round(traffic / row[leg]["median_us"] / PEAK_BYTES_PER_US, 3)
        emit(row)
        del chains


if __name__ == "__main__":
    main()
