"""What the sRGB colour kind of the mip filters costs (ITW_MIP_SRGB; include/itw_dispatch.h "Mip chains"), in the method of
tools/mipgen_timing.py: a call = itwGenerateMipChain followed by a synchronise of the stream, inside a host clock; the legs of a row
alternate call by call in one run; per leg the median of reps x inner calls (default 7 x 5 = 35), the fastest call, p10 and p90 -- the
run's own spread.

Rows (one JSON object per line; stdout, and appended to profiles/srgb_mip_timing.jsonl unless --no-save), full RGBA8 chains, device-resident:
  2d_4096, cube_1024      legs plain_pyramid, plain_per_level, srgb_pyramid, srgb_per_level; `srgb_over_plain_*` = the medians' ratio with
                          the spread as [p10 / p90, p90 / p10]; `srgb_pyramid_over_srgb_per_level` decides the flag's default route
--plain-only              only the two plain legs: what a build without the flag can run.  With --lib=PATH the library under the clock is
                          that file (another build of libispc_texcomp.so), loaded in place of the tree's.
Usage: python tools/srgb_mip_timing.py [reps] [inner] [--label=TEXT] [--no-save] [--out=PATH] [--only=SUBSTRING] [--plain-only] [--lib=PATH]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
import numpy as np                      # noqa: E402
import itw_amd                          # noqa: E402

MIP_PER_LEVEL, MIP_SRGB = 1, 4


def opt(name, default):
    return next((a[len(name) + 3:] for a in sys.argv if a.startswith("--" + name + "=")), default)


def measure(legs, reps, inner, stream):
    for _ in range(3):                                            # warm-up: code objects, the thread's buffers, clocks
        for _, call in legs:
            assert call() == 0
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


def ratio(a, b):
    return {"median": round(a["median_us"] / b["median_us"], 3), "spread": [round(a["p10_us"] / b["p90_us"], 3), round(a["p90_us"] / b["p10_us"], 3)]}


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    inner = int(args[1]) if len(args) > 1 else 5
    only = opt("only", "")
    plain_only = "--plain-only" in sys.argv
    out_path = opt("out", os.path.join(ROOT, "profiles", "srgb_mip_timing.jsonl"))
    lib_path = opt("lib", "")
    L = C.CDLL(os.path.abspath(lib_path), mode=C.RTLD_GLOBAL) if lib_path else itw_amd.lib()       # (an older build lacks what the binding's loader names)
    L.itwSetStream.argtypes, L.itwSetStream.restype = [C.c_void_p], None
    L.itwGenerateMipChain.argtypes, L.itwGenerateMipChain.restype = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32], C.c_int
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    L.itwSetStream(stream.cuda_stream)
    L.itwDeviceInfo.restype = C.c_char_p

    for name, w, h, items in (("2d_4096", 4096, 4096, 1), ("cube_1024", 1024, 1024, 6)):
        if only not in name:
            continue
        n = int(L.itwMipLevels(w, h))
        chains = []
        for i in range(items):
            base = torch.from_numpy(np.random.default_rng(10 + i).integers(0, 256, (h, w, 4), dtype=np.uint8)).to(dev)
            chains.append([base] + [torch.empty((max(1, h >> l), max(1, w >> l), 4), dtype=torch.uint8, device=dev) for l in range(1, n)])
        arr = C.cast(itw_amd.abi._surfaces([lv for ch in chains for lv in ch]), C.c_void_p)
        call = lambda flags: (lambda: L.itwGenerateMipChain(arr, items, n, 4, flags))
        legs = [("plain_pyramid", call(0)), ("plain_per_level", call(MIP_PER_LEVEL))]
        if not plain_only:
            legs += [("srgb_pyramid", call(MIP_SRGB)), ("srgb_per_level", call(MIP_SRGB | MIP_PER_LEVEL))]
        row = {"row": name, "width": w, "height": h, "items": items, "levels": n, "library": "another build (--lib)" if lib_path else "the tree's"}
        row.update(measure(legs, reps, inner, stream))
        if not plain_only:
            row["srgb_over_plain_pyramid"] = ratio(row["srgb_pyramid"], row["plain_pyramid"])
            row["srgb_over_plain_per_level"] = ratio(row["srgb_per_level"], row["plain_per_level"])
            row["srgb_pyramid_over_srgb_per_level"] = ratio(row["srgb_pyramid"], row["srgb_per_level"])
        row.update({"reps": reps, "inner": inner, "calls_per_leg": reps * inner, "label": opt("label", ""), "device": L.itwDeviceInfo().decode(),
                    "unit": "us per call, host clock around the call + stream synchronise"})
        print(json.dumps(row), flush=True)
        if "--no-save" not in sys.argv:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "a") as f:
                f.write(json.dumps(row) + "\n")
        del chains


if __name__ == "__main__":
    main()
