"""One run of the BC7 launcher's timing rows against the build under ROOT (a checkout with its libraries built): device-resident BC7 `basic`,
`slow`, `alpha_basic` and `alpha_slow` at 64^2, 512^2, 2048^2 and 4096^2 -- small calls are where host-side cost shows -- and `slow` 4096^2 as
one host-pointer call.  Per row the median and best of N calls and the first 16 hex digits of the output's SHA-256, one JSON object per line
(stdout, and appended to OUT_JSONL).  Two builds are compared by running this file once per build and run, alternating
(profiles/bc7_launcher_refactor_timing.jsonl); the method is tools/host_layer_timing.py's.
Usage: python tools/bc7_launcher_timing.py ROOT BUILD_TAG RUN_INDEX OUT_JSONL [calls=35]"""
import ctypes as C
import hashlib
import json
import os
import sys
import time

ROOT, TAG, RUN, OUT = os.path.abspath(sys.argv[1]), sys.argv[2], int(sys.argv[3]), sys.argv[4]
CALLS = int(sys.argv[5]) if len(sys.argv) > 5 else 35
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
import numpy as np                      # noqa: E402
import torch                            # noqa: E402
import itw_amd                          # noqa: E402
from itw_amd import surfaces            # noqa: E402

assert os.path.abspath(itw_amd.lib_path()).startswith(ROOT), itw_amd.lib_path()
PROFILES = ("basic", "slow", "alpha_basic", "alpha_slow")
SIZES = (64, 512, 2048, 4096)


def median_ms(fn, sync):
    fn(); sync(); fn(); sync()
    ts = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        fn(); sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    L = itw_amd.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rows = []

    def emit(row, med, best, out):
        data = out.cpu().numpy() if hasattr(out, "cpu") else out
        rows.append({"build": TAG, "run": RUN, "row": row, "median_ms": round(med, 4), "best_ms": round(best, 4), "calls": CALLS,
                     "sha256_16": hashlib.sha256(data.tobytes()).hexdigest()[:16]})
        print(json.dumps(rows[-1]), flush=True)

    full = surfaces.ldr_smooth(4096, 4096)
    translucent = full.copy()
    translucent[:, 1024:3072, 3] = translucent[:, 1024:3072, 0]          # the alpha profiles: opaque and translucent columns
    for size in SIZES:
        for prof in PROFILES:
            img = np.ascontiguousarray((translucent if prof.startswith("alpha") else full)[:size, :size])
            d = torch.from_numpy(img).to(dev)
            out = itw_amd.compress("bc7", d, prof)
            med, best = median_ms(lambda: itw_amd.compress("bc7", d, prof, out=out), torch.cuda.synchronize)
            emit(f"device {size}^2 bc7 {prof}", med, best, out)
    s7 = itw_amd.bc7_profile("slow")
    surf = itw_amd.RgbaSurface(full.ctypes.data, 4096, 4096, full.strides[0])
    out = np.zeros(1024 * 1024 * 16, np.uint8)
    med, best = median_ms(lambda: L.CompressBlocksBC7(C.byref(surf), out.ctypes.data, C.byref(s7)), lambda: None)
    emit("one call 4096^2 host bc7 slow", med, best, out)
    with open(OUT, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


main()
