"""ETC1 at fastSkipTreshold 1, 6 and 32 against BC1 and BC7 `basic` of the same build, device-resident 4096^2 (or --size=N), one run: the
legs alternate call by call, so that whatever the clocks do they do to all of them.

A call = the entry point on device pointers followed by a synchronise of its stream, inside a host clock (time.perf_counter): what a
caller waiting for the blocks sees.  Everything is warmed up first.  Per leg: the median of reps x inner calls (default 7 x 5 = 35), the
fastest call, and the spread as (p90 - p10) / median.

For scale, the reference library's time for the same surface cut to 512^2 (oracle/_ref/libispc_texcomp_ref_full.so, where build() made
it): 16 host threads over row bands, one call per threshold.  That library is a SCALAR build of the reference, not ISPC SIMD: it says what
the checker costs, not what the reference's shipped object code would.

One JSON object per line (stdout, and appended to profiles/etc1_timing.jsonl unless --no-save).
Usage: python tools/etc1_timing.py [reps] [inner] [--size=N] [--label=TEXT] [--no-save] [--out=PATH] [--no-reference]"""
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
import numpy as np                      # noqa: E402
import itw_amd                          # noqa: E402
from itw_amd import surfaces           # noqa: E402

THRESHOLDS = (1, 6, 32)
REF_THREADS = 16


def opt(name, default):
    return next((a[len(name) + 3:] for a in sys.argv if a.startswith("--" + name + "=")), default)


def reference_leg(img):
    """ms per 512^2 call of the reference library at each threshold, on REF_THREADS host threads by row bands; None where it is not built"""
    path = os.path.join(ROOT, "oracle", "_ref", "libispc_texcomp_ref_full.so")
    if not os.path.exists(path):
        return None
    R = C.CDLL(path, mode=os.RTLD_LOCAL)
    h, w = img.shape[:2]
    rows = [(h // 4) * i // REF_THREADS * 4 for i in range(REF_THREADS + 1)]
    out = np.zeros((h // 4) * (w // 4) * 8, dtype=np.uint8)
    res = {}
    for t in THRESHOLDS:
        st = itw_amd.EtcSettings(t)

        def band(i):
            surf = itw_amd.RgbaSurface(img.ctypes.data + rows[i] * img.strides[0], w, rows[i + 1] - rows[i], img.strides[0])
            R.CompressBlocksETC1(C.byref(surf), C.c_void_p(out.ctypes.data + (rows[i] // 4) * (w // 4) * 8), C.byref(st))

        t0 = time.perf_counter()
        with ThreadPoolExecutor(REF_THREADS) as ex:
            list(ex.map(band, range(REF_THREADS)))
        res[f"t{t}_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    return res


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    inner = int(args[1]) if len(args) > 1 else 5
    size = int(opt("size", 4096))
    out_path = opt("out", os.path.join(ROOT, "profiles", "etc1_timing.jsonl"))
    L = itw_amd.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    L.itwSetStream(stream.cuda_stream)
    img = surfaces.ldr_smooth(size, size)
    src = torch.from_numpy(img).to(dev)
    surf = itw_amd.RgbaSurface(src.data_ptr(), size, size, size * 4)
    blocks = (size // 4) ** 2
    out8 = torch.empty(blocks * 8, dtype=torch.uint8, device=dev)
    out16 = torch.empty(blocks * 16, dtype=torch.uint8, device=dev)
    basic = itw_amd.bc7_profile("basic")
    etc = {t: itw_amd.EtcSettings(t) for t in THRESHOLDS}
    calls = [(f"etc1_t{t}", (lambda t=t: L.itwCompressBlocksETC1(C.byref(surf), out8.data_ptr(), C.byref(etc[t])))) for t in THRESHOLDS]
    calls.append(("bc1", lambda: L.CompressBlocksBC1(C.byref(surf), out8.data_ptr())))
    calls.append(("bc7_basic", lambda: L.CompressBlocksBC7(C.byref(surf), out16.data_ptr(), C.byref(basic))))
    for _ in range(3):                                            # warm-up: code objects, workspace, clocks
        for _, fn in calls:
            fn()
    stream.synchronize()
    times = {name: [] for name, _ in calls}
    for _ in range(reps):
        for _ in range(inner):
            for name, fn in calls:                                # the legs alternate
                t0 = time.perf_counter()
                fn()
                stream.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e6)
    row = {"size": size, "reps": reps, "inner": inner, "calls_per_leg": reps * inner, "label": opt("label", ""),
           "device": L.itwDeviceInfo().decode(), "unit": "us per call, host clock around call + stream synchronise"}
    for name, t in times.items():
        t = np.sort(np.array(t))
        med = float(np.median(t))
        row[name] = {"median_us": round(med, 1), "min_us": round(float(t[0]), 1),
                     "spread": round(float(np.percentile(t, 90) - np.percentile(t, 10)) / med, 3),
                     "mpix_per_s": round(size * size / med, 1)}
    for t in THRESHOLDS:
        row[f"etc1_t{t}_over_bc7_basic"] = round(row[f"etc1_t{t}"]["median_us"] / row["bc7_basic"]["median_us"], 2)
    if "--no-reference" not in sys.argv:
        cut = min(512, size)
        ref = reference_leg(np.ascontiguousarray(img[:cut, :cut]))
        row["reference_512"] = ({"what": f"scalar build of the reference, not ISPC SIMD; {cut}^2 cut of the same surface, {REF_THREADS} host threads by row bands, one call",
                                 **ref} if ref else "oracle/_ref is not built here: not measured")
    print(json.dumps(row), flush=True)
    if "--no-save" not in sys.argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
