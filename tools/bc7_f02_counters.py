"""VALU instructions per kernel of a BC7 `slow` call at 4096^2 on the bench surface, from a counter pass of its own (no tracing alongside):

    rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES --output-format csv -d OUT -o pmc -- python tools/bc7_f02_counters.py run
    python tools/bc7_f02_counters.py table OUT/**/pmc_counter_collection.csv

`run` makes CALLS device-resident calls and nothing else; `table` prints one line per BC7 kernel in the layout of profiles/r11_bc7_insts_valu.txt."""
import csv
import os
import re
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = 4
SIZE = 4096


def run():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "intel-texture-works-plugin_amd")]
    import torch
    import itw_amd
    from itw_amd import surfaces
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    img = torch.from_numpy(surfaces.ldr_smooth(SIZE, SIZE)).to(dev)
    out = torch.empty(SIZE * SIZE, dtype=torch.uint8, device=dev)
    for _ in range(CALLS):
        itw_amd.compress("bc7", img, "slow", out=out)
        torch.cuda.synchronize()


def table(path):
    per = defaultdict(lambda: defaultdict(float))            # kernel -> counter -> sum over dispatches
    dispatches = defaultdict(set)
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        if "bc7" not in name:
            continue
        name = re.sub(r"\(.*", "", re.sub(r"^void ", "", name))
        name = re.sub(r"^itw::(?=bc7_\w+<)", "", name)
        per[name][r["Counter_Name"]] += float(r["Counter_Value"])
        dispatches[name].add(r["Dispatch_Id"])
    total = 0.0
    for name in sorted(per, key=lambda n: -per[n]["SQ_INSTS_VALU"]):
        valu, waves = per[name]["SQ_INSTS_VALU"], per[name]["SQ_WAVES"]
        total += valu
        print(f"{name:44s} {len(dispatches[name]) / CALLS:4.1f} dispatches/call {valu / CALLS / 1e6:14.2f} M SQ_INSTS_VALU per call "
              f"{waves / CALLS:10.0f} waves {valu / waves if waves else 0:10.0f} per wave")
    print(f"all BC7 kernels of a call {total / CALLS / 1e6:32.1f} M SQ_INSTS_VALU per call")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run()
    else:
        table(sys.argv[2])
