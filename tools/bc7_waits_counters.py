"""The surfaces of tests/test_gpu_bc7_waits.py and what a build's RGB bounded order counts on them (GPU).

    python tools/bc7_waits_counters.py OUT.json

encodes every surface below with BC7 `slow` through the PRODUCT library of the tree it is run from, deep path, with the pilot's threshold left to
itself, forced to 0 and forced to 100, under ITW_BC7_PILOT_DEBUG=1, and writes what the library printed -- the pilot's two counts and verdict, the
six rotation lists, the blocks listed for modes 1/3, the pairs, the overflow words and the deferred blocks, per band -- as JSON.  Run from a checkout
of the PARENT commit it gives tests/golden/bc7_waits_parent_counters.json: the counts are properties of the content and of the routes' rules, not of
how a kernel claims its list stretches, so a build that only takes waits out has to reproduce every one of them.
"""
import json
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((516, 604), (1024, 2048))          # rows x columns: 76.1 chunks of 256 blocks (a ragged last chunk) and 512 chunks
CONTENTS = ("smooth", "flat", "baboon")
PILOTS = (None, 0, 100)
FLAT = (37, 120, 201, 255)


def baboon_base(golden_inputs):
    b = golden_inputs["baboon"]
    return np.ascontiguousarray(b[:b.shape[0] // 4 * 4, :b.shape[1] // 4 * 4])


def tile_to(base, h, w):
    """`base` (sides multiples of 4) repeated and cut to h x w (multiples of 4): blocks stay whole"""
    ry, rx = -(-h // base.shape[0]), -(-w // base.shape[1])
    return np.ascontiguousarray(np.tile(base, (ry, rx, 1))[:h, :w])


def tile_blocks_to(blocks, base_shape, h, w):
    """the 16-byte blocks of tile_to(base, h, w) from the blocks of `base`"""
    by, bx = base_shape[0] // 4, base_shape[1] // 4
    g = np.asarray(blocks, np.uint8).reshape(by, bx, 16)
    ry, rx = -(-(h // 4) // by), -(-(w // 4) // bx)
    return np.ascontiguousarray(np.tile(g, (ry, rx, 1))[:h // 4, :w // 4]).reshape(-1)


def surface(name, golden_inputs, h, w):
    from itw_amd import surfaces
    if name == "smooth":
        return surfaces.ldr_smooth(h, w)                       # the bench surface's generator
    if name == "flat":
        img = np.empty((h, w, 4), np.uint8)
        img[...] = FLAT
        return img
    if name == "baboon":
        return tile_to(baboon_base(golden_inputs), h, w)
    raise ValueError(name)


def key(name, h, w, pilot):
    return f"{name}/{h}x{w}/pilot={'auto' if pilot is None else pilot}"


_PILOT = re.compile(r"bc7 pilot: estimate (\d+) of (\d+) sampled blocks listed -> (bounded|reference order); lists (\d+) \+ (\d+) of")
_ROT = re.compile(r"bc7 rot tasks: rotation lists (\d+) / (\d+) / (\d+) \(band 0\) \+ (\d+) / (\d+) / (\d+) \(band 1\)")
_PAIRS = re.compile(r"bc7 pairs: band (\d): (\d+) pairs, fullest bucket \d+ of \d+, overflow (\d+), deferred to the full scan (\d+)")


def parse(text):
    """one call's ITW_BC7_PILOT_DEBUG lines -> the counters by itw_amd.abi.BC7_CALL_COUNTERS' names"""
    p, r = _PILOT.search(text), _ROT.search(text)
    out = {"pilot_listed": int(p.group(1)), "pilot_sampled": int(p.group(2)), "pilot_flag": 1 if p.group(3) == "bounded" else 0,
           "listed0": int(p.group(4)), "listed1": int(p.group(5))}
    for i, n in enumerate(("rot00", "rot01", "rot02", "rot10", "rot11", "rot12")):
        out[n] = int(r.group(i + 1))
    for m in _PAIRS.finditer(text):
        k = m.group(1)
        out["pairs" + k], out["overflow" + k], out["redo" + k] = int(m.group(2)), int(m.group(3)), int(m.group(4))
    return out


def main(out_path):
    os.environ["ITW_BC7_PILOT_DEBUG"] = "1"                   # read once per process, before the first call
    sys.path[:0] = [ROOT, os.path.join(ROOT, "intel-texture-works-plugin_amd")]
    import torch
    import itw_amd
    gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "inputs.npz")))
    dev = torch.device("cuda:0")
    itw_amd.set_bc7_path("deep")
    result = {}
    for h, w in SIZES:
        for name in CONTENTS:
            src = torch.from_numpy(surface(name, gold, h, w)).to(dev)
            for pilot in PILOTS:
                itw_amd.set_bc7_pilot(pilot)
                with tempfile.TemporaryFile() as f:
                    saved = os.dup(2)
                    os.dup2(f.fileno(), 2)
                    try:
                        itw_amd.compress("bc7", src, "slow")
                        torch.cuda.synchronize()
                    finally:
                        os.dup2(saved, 2)
                        os.close(saved)
                    f.seek(0)
                    result[key(name, h, w, pilot)] = parse(f.read().decode())
    with open(out_path, "w") as f:
        json.dump({"what": "BC7 slow, deep path, the product library of the commit before the rotation lists were claimed per workgroup: "
                           "ITW_BC7_PILOT_DEBUG's counters per surface and pilot threshold (tools/bc7_waits_counters.py)", "counters": result}, f, indent=1, sort_keys=True)
    print("wrote", out_path, len(result), "records")


if __name__ == "__main__":
    main(sys.argv[1])
