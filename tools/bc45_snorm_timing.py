"""BC4 / BC5 against BC4_SNORM / BC5_SNORM, device-resident 4096^2 (or --size=N), one run: the legs alternate call by call, so that
whatever the clocks do they do to all of them.  The signed legs encode the UNORM surface XOR 0x80: the same blocks, code for code, in
signed order (0 -> -128, 255 -> 127), so both pairs meet the same ramp forms and iteration counts.

A call = CompressBlocks* on device pointers followed by a synchronise of its stream, inside a host clock (time.perf_counter): what a
caller waiting for the blocks sees.  Everything is warmed up first (index tables, code objects).  Per leg: the median of reps x inner
calls (default 7 x 5), the fastest call, and the spread as (p90 - p10) / median.

Where the library has no signed entry points (a build of an earlier commit: --lib=PATH loads another libispc_texcomp.so; say which with
--label) only the UNORM legs run, which is how UNORM on this commit is compared with UNORM before it.

One JSON object per line (stdout, and appended to profiles/bc45_snorm_timing.jsonl unless --no-save).
Usage: python tools/bc45_snorm_timing.py [reps] [inner] [--size=N] [--lib=PATH] [--label=TEXT] [--no-save] [--out=PATH]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
import numpy as np                      # noqa: E402
from itw_amd import surfaces           # noqa: E402


class Surface(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32)]


def opt(name, default):
    return next((a[len(name) + 3:] for a in sys.argv if a.startswith("--" + name + "=")), default)


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    inner = int(args[1]) if len(args) > 1 else 5
    size = int(opt("size", 4096))
    path = opt("lib", os.path.join(ROOT, "intel-texture-works-plugin_amd", "lib", "libispc_texcomp.so"))
    out_path = opt("out", os.path.join(ROOT, "profiles", "bc45_snorm_timing.jsonl"))
    L = C.CDLL(path)
    L.itwSetStream.argtypes = [C.c_void_p]
    L.itwSetStream.restype = None
    L.itwDeviceInfo.restype = C.c_char_p
    legs = [("bc4", "CompressBlocksBC4", 8, False), ("bc5", "CompressBlocksBC5", 16, False)]
    if hasattr(L, "CompressBlocksBC4S") and hasattr(L, "CompressBlocksBC5S"):
        legs += [("bc4_snorm", "CompressBlocksBC4S", 8, True), ("bc5_snorm", "CompressBlocksBC5S", 16, True)]
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    L.itwSetStream(stream.cuda_stream)
    unorm = surfaces.ldr_smooth(size, size)
    src = {False: torch.from_numpy(unorm).to(dev), True: torch.from_numpy(unorm ^ 0x80).to(dev)}
    calls = []
    for name, sym, bpb, signed in legs:
        fn = getattr(L, sym)
        fn.argtypes = [C.POINTER(Surface), C.c_void_p]
        fn.restype = None
        out = torch.empty((size // 4) ** 2 * bpb, dtype=torch.uint8, device=dev)
        surf = Surface(src[signed].data_ptr(), size, size, size * 4)
        calls.append((name, fn, surf, out))
    L.itwWarmupBC45()
    if len(legs) > 2:
        L.itwWarmupBC45S()
    for _ in range(5):                                            # warm-up: code objects, clocks
        for _, fn, surf, out in calls:
            fn(C.byref(surf), out.data_ptr())
    stream.synchronize()
    times = {name: [] for name, *_ in calls}
    for _ in range(reps):
        for _ in range(inner):
            for name, fn, surf, out in calls:                     # the legs alternate
                t0 = time.perf_counter()
                fn(C.byref(surf), out.data_ptr())
                stream.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e6)
    row = {"size": size, "reps": reps, "inner": inner, "calls_per_leg": reps * inner, "library": "this tree's" if opt("lib", None) is None else "--lib " + os.path.basename(path),
           "label": opt("label", ""), "device": L.itwDeviceInfo().decode(), "unit": "us per call, host clock around call + stream synchronise"}
    for name, t in times.items():
        t = np.sort(np.array(t))
        med = float(np.median(t))
        row[name] = {"median_us": round(med, 2), "min_us": round(float(t[0]), 2),
                     "spread": round(float(np.percentile(t, 90) - np.percentile(t, 10)) / med, 3)}
    for s, u in (("bc4_snorm", "bc4"), ("bc5_snorm", "bc5")):
        if s in row:
            row[s + "_over_" + u] = round(row[s]["median_us"] / row[u]["median_us"], 3)
    print(json.dumps(row), flush=True)
    if "--no-save" not in sys.argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
