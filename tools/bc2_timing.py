"""BC2 (DirectXTex's D3DXEncodeBC2, csrc/bc2.hip) timed on the project's method, as tools/bc1a_timing.py times BC1A: a call = the entry point
followed by a synchronise of its stream, inside a host clock (time.perf_counter); the legs of a group alternate call by call in one job;
per leg the median of reps x inner calls (default 7 x 5 = 35), the fastest call and the p10-p90 spread over the median.  Run it twice
(--label=run1 / run2): the difference between two runs is the noise floor of every comparison made here.

Groups (one JSON object per line on stdout, appended to profiles/bc2_timing.jsonl unless --no-save):
  resident  4096^2 (--size=N) cut-out content, device-resident, through itwCompressImageSlicedEx with one slice: BC2 plain, uniform, dither
            RGB, dither A, all flags; beside them, in the same build and job, BC1A plain (the same colour search, 8 bytes fewer stored)
            and the ISPC BC3 kernel.  Rows carry Mpix/s; the BC2 rows the share of HBM peak their traffic (4 B read per texel + 1 B written)
            comes to and the ratios to the BC1A and BC3 medians of the same run.
  sliced    one row: BC2 plain from pageable host memory in 64 slices with a progress callback.
Usage: python tools/bc2_timing.py [reps] [inner] [--size=N] [--groups=resident,sliced] [--label=TEXT] [--no-save]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np                      # noqa: E402
import itw_amd                          # noqa: E402
from bc1a_timing import HBM_PEAK_GBS, alternate, cutout, opt, sliced_call      # noqa: E402


def main():
    import torch
    nums = [int(a) for a in sys.argv[1:] if a.isdigit()]
    reps, inner = nums[0] if nums else 7, nums[1] if len(nums) > 1 else 5
    size = int(opt("size", "4096"))
    groups = opt("groups", "resident,sliced").split(",")
    label = opt("label", "")
    out_path = os.path.join(ROOT, "profiles", "bc2_timing.jsonl")
    L = itw_amd.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.itwSetStream(torch.cuda.current_stream(dev).cuda_stream)
    sync = torch.cuda.synchronize
    img = cutout(size)
    mpix = size * size / 1e6
    rows = []

    def row(group, name, s, extra=None):
        r = {"tool": "bc2_timing", "group": group, "leg": name, "size": size, "reps": reps * inner, "label": label, "device": itw_amd.device_info(), **s,
             "mpix_s": round(mpix / (s["median_us"] * 1e-6), 1)}
        r.update(extra or {})
        rows.append(r)
        print(json.dumps(r), flush=True)

    S = itw_amd.Bc1aSettings
    if "resident" in groups:
        d_img = torch.from_numpy(img).to(dev)
        d_out = torch.empty(size * size, dtype=torch.uint8, device=dev)             # 16-byte blocks fit
        surf = itw_amd.RgbaSurface(d_img.data_ptr(), size, size, size * 4)
        spec = [("bc2", "bc2", S()), ("bc2_uniform", "bc2", S(uniform=True)), ("bc2_dither_rgb", "bc2", S(dither_rgb=True)),
                ("bc2_dither_a", "bc2", S(dither_a=True)), ("bc2_all_flags", "bc2", S(0.5, True, True, True)),
                ("bc1a", "bc1a", S()), ("bc3_ispc", "bc3", None)]
        legs = [(name, sliced_call(L, fmt, st, surf, d_out.data_ptr(), size, 1 << 62, None)) for name, fmt, st in spec]
        res = alternate(legs, reps, inner, sync)
        for name, s in res.items():
            extra = None
            if name.startswith("bc2"):
                extra = {"hbm_share": round(size * size * 5.0 / (s["median_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                         "over_bc1a": round(s["median_us"] / res["bc1a"]["median_us"], 3), "over_bc3_ispc": round(s["median_us"] / res["bc3_ispc"]["median_us"], 3)}
            row("resident", name, s, extra)
    if "sliced" in groups:
        out = np.empty(size * size, dtype=np.uint8)
        cb = itw_amd.PROGRESS_FUNC(lambda i, n, u: True)
        surf = itw_amd.RgbaSurface(img.ctypes.data, size, size, size * 4)
        st = S()
        legs = [("bc2", sliced_call(L, "bc2", st, surf, out.ctypes.data, size, size * size // 64, C.cast(cb, C.c_void_p)))]
        for name, s in alternate(legs, reps, inner, sync).items():
            row("sliced_host_64", name, s)
    if "--no-save" not in sys.argv and rows:
        with open(out_path, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
