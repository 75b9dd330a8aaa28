"""What the free-size chain costs (ITW_MIP_RESIZE; include/itw_dispatch.h "Mip chains: free sizes"; csrc/resize.hip), in the method of
tools/mip_filter_timing.py: a call = the entry point followed by a synchronise of the stream, inside a host clock (time.perf_counter); the
legs of a row alternate call by call in one run; per leg the median of reps x inner calls (default 7 x 5 = 35), the fastest call, p10 and
p90 -- the run's own spread.  Run it twice.

Rows (one JSON object per line; stdout, and appended to profiles/resize_timing.jsonl unless --no-save), device-resident two-level chains,
each for RGBA16F and RGBA8:
  4096_to_1024, 4096_to_256          `triangle` (the rows of profiles/resize_timing.jsonl labelled run1 / run2 also hold `triangle_gather`
                                     and `triangle_staged`: the gather against a kernel that staged source rows in LDS, which lost on
                                     every row and was removed with its switch; `triangle_gather` is what `triangle` runs now)
  4096_to_2048                       `cubic`
  4000x3000_to_4096                  `linear`, `cubic`
  1024_to_4096                       `cubic`, `point`
Every leg also as a share of 8 TB/s over `bytes`: the source read once and the target written once, what the call has to move.
Usage: python tools/resize_timing.py [reps] [inner] [--label=TEXT] [--no-save] [--out=PATH] [--only=SUBSTRING]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import itw_amd                          # noqa: E402
from mip_filter_timing import PEAK_BYTES_PER_US, content, measure, opt      # noqa: E402

ROWS = [("4096_to_1024", (4096, 4096), (1024, 1024), ("triangle",)),
        ("4096_to_256", (4096, 4096), (256, 256), ("triangle",)),
        ("4096_to_2048", (4096, 4096), (2048, 2048), ("cubic",)),
        ("4000x3000_to_4096", (4000, 3000), (4096, 4096), ("linear", "cubic")),
        ("1024_to_4096", (1024, 1024), (4096, 4096), ("cubic", "point"))]
LEGS = ("triangle", "cubic", "linear", "point")


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    inner = int(args[1]) if len(args) > 1 else 5
    only = opt("only", "")
    out_path = opt("out", os.path.join(ROOT, "profiles", "resize_timing.jsonl"))
    T = itw_amd.test_lib()              # the product's sources with the hooks: every leg runs through one library
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    T.itwSetStream(stream.cuda_stream)

    def checked(arr, px, flags):
        def call():
            if T.itwGenerateMipChain(arr, 1, 2, px, flags) != 0:
                raise RuntimeError("itwGenerateMipChain failed: " + (itw_amd.last_error() or ""))
        return call

    for name, (sw, sh), (dw, dh), legs in ROWS:
        for half in (True, False):
            row_name = name + ("_rgba16f" if half else "_rgba8")
            if only not in row_name:
                continue
            px = 8 if half else 4
            base = torch.from_numpy(content(sh, sw, half, 10)).to(dev)
            chain = [base, torch.empty((dh, dw, 4), dtype=base.dtype, device=dev)]
            arr = C.cast(itw_amd.abi._surfaces(chain), C.c_void_p)
            traffic = (sw * sh + dw * dh) * px
            assert all(leg in LEGS for leg in legs)
            calls = [(leg, checked(arr, px, itw_amd.resize_flags(leg))) for leg in legs]
            row = {"row": row_name, "source": [sw, sh], "target": [dw, dh], "pixel_size": px, "bytes": traffic}
            row.update(measure(calls, reps, inner, stream))
            for leg in legs:
                row[leg + "_fraction_of_8TBs"] = round(traffic / row[leg]["median_us"] / PEAK_BYTES_PER_US, 3)
            row.update({"reps": reps, "inner": inner, "calls_per_leg": reps * inner, "label": opt("label", ""), "device": itw_amd.device_info(),
                        "unit": "us per call, host clock around the call + stream synchronise"})
            print(json.dumps(row), flush=True)
            if "--no-save" not in sys.argv:
                os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
                with open(out_path, "a") as f:
                    f.write(json.dumps(row) + "\n")
            del chain, base


if __name__ == "__main__":
    main()
