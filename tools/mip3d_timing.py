"""What the volume mip chain costs (itwGenerateMipChain with ITW_MIP_VOLUME; include/itw_dispatch.h "Mip chains: volumes"; csrc/mip3d.hip), in the method of
tools/mip_filter_timing.py: a call = the entry point followed by a synchronise of the stream, inside a host clock (time.perf_counter); the
legs of a row alternate call by call in one run, so that whatever the clocks do they do to all of them; per leg the median of reps x inner
calls (default 7 x 5 = 35), the fastest call, p10 and p90 -- the run's own spread.  Run it twice.

Rows (one JSON object per line; stdout, and appended to profiles/mip3d_timing.jsonl unless --no-save), device-resident full chains:
  vol_256_rgba16f / _rgba8, vol_128_..., vol_64x64x16_...   `box` (the default of a power-of-two volume: one launch per level), then `point`,
           `linear`, `cubic`, `triangle`
  vol_100x60x40_rgba16f                                      the default is `triangle`; `point`, `linear`, `cubic` beside it
Every leg also as a multiple of the row's first leg, and as a share of 8 TB/s over `bytes_per_level`: every level but the last read once
and every level but the base written once, what a one-launch-per-level route moves at the least.  `launches` is levels - 1 for every leg:
the library has one route per filter.
The rows of profiles/mip3d_timing.jsonl labelled run1 / run2 were recorded while the box filter still had a brick route: their `per_level` leg is
this tool's `box`, and their `brick`, `brick_gain_us`, `legs_spread_us` and `brick_wins` fields are that route's, since removed.
Usage: python tools/mip3d_timing.py [reps] [inner] [--label=TEXT] [--no-save] [--out=PATH] [--only=SUBSTRING]"""
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


def content(d, h, w, half, seed):
    rng = np.random.default_rng(seed)
    if half:
        return rng.random((d, h, w, 4), dtype=np.float32).astype(np.float16).view(np.int16)
    return rng.integers(0, 256, (d, h, w, 4), dtype=np.uint8)


def measure(legs, reps, inner, stream):
    for _ in range(3):                                            # warm-up: code objects, the thread's buffers, the triangle lists, clocks
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
    out_path = opt("out", os.path.join(ROOT, "profiles", "mip3d_timing.jsonl"))
    L = itw_amd.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    L.itwSetStream(stream.cuda_stream)

    def emit(row):
        row.update({"reps": reps, "inner": inner, "calls_per_leg": reps * inner, "label": opt("label", ""), "device": itw_amd.device_info(),
                    "unit": "us per call, host clock around the call + stream synchronise"})
        print(json.dumps(row), flush=True)
        if "--no-save" not in sys.argv:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "a") as f:
                f.write(json.dumps(row) + "\n")

    def checked(arr, depth, n, px, flags):
        def call():
            if L.itwGenerateMipChain(arr, depth, n, px, flags | itw_amd.MIP_VOLUME) != 0:
                raise RuntimeError("itwGenerateMipChain refused the volume: " + (itw_amd.last_error() or ""))
        return call

    sizes = (("vol_256", 256, 256, 256), ("vol_128", 128, 128, 128), ("vol_64x64x16", 64, 64, 16))
    rows = [(f"{name}_{kind}", w, h, d, kind == "rgba16f") for name, w, h, d in sizes for kind in ("rgba16f", "rgba8")] + [("vol_100x60x40_rgba16f", 100, 60, 40, True)]
    for name, w, h, d, half in rows:
        if only not in name:
            continue
        n = itw_amd.mip_levels_3d(w, h, d)
        base = torch.from_numpy(content(d, h, w, half, 10)).to(dev)
        levels = [base] + [torch.empty((max(1, d >> l), max(1, h >> l), max(1, w >> l), 4), dtype=base.dtype, device=dev) for l in range(1, n)]
        px = 8 if half else 4
        arr = C.cast(itw_amd.abi._surfaces([lv[z] for lv in levels for z in range(lv.shape[0])]), C.c_void_p)
        texels = [max(1, w >> l) * max(1, h >> l) * max(1, d >> l) * px for l in range(n)]
        traffic = sum(texels[l - 1] + texels[l] for l in range(1, n))
        box = all(v & (v - 1) == 0 for v in (w, h, d))
        legs = [("box" if box else "triangle", checked(arr, d, n, px, 0)), ("point", checked(arr, d, n, px, itw_amd.MIP_POINT)),
                ("linear", checked(arr, d, n, px, itw_amd.MIP_LINEAR)), ("cubic", checked(arr, d, n, px, itw_amd.MIP_CUBIC))]
        if box:
            legs.append(("triangle", checked(arr, d, n, px, itw_amd.MIP_TRIANGLE)))
        row = {"row": name, "width": w, "height": h, "depth": d, "levels": n, "launches": n - 1, "pixel_size": px, "bytes_per_level": traffic,
               "default_filter": legs[0][0]}
        row.update(measure(legs, reps, inner, stream))
        for leg, _ in legs:
            row[leg + "_over_" + legs[0][0]] = round(row[leg]["median_us"] / row[legs[0][0]]["median_us"], 3)
            row[leg + "_fraction_of_8TBs"] = round(traffic / row[leg]["median_us"] / PEAK_BYTES_PER_US, 3)
        emit(row)
        del levels, base


if __name__ == "__main__":
    main()
