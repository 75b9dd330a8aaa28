#!/usr/bin/env python3
"""Writes tests/golden/golden_bc45_snorm.npz: seeded RGBA8_SNORM inputs and the streams the reference's own D3DXEncodeBC4S / D3DXEncodeBC5S
give them (tests/_dxtex_snorm.py: oracle/_ref/libdxtex_bc_ref.so, built by __graft_entry__.build() from the reference tree).  The GPU
suite compares against the file, so that check needs neither the binary nor the tree.

    python tools/gen_golden_bc45_snorm.py [--check]      --check: compare with the committed file instead of writing it
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "intel-texture-works-plugin_amd")):
    sys.path.insert(0, p)
PATH = os.path.join(ROOT, "tests", "golden", "golden_bc45_snorm.npz")


def build():
    import _dxtex_snorm as ref
    from itw_amd import surfaces
    out = {}
    for name, img in (("normal_53x101", surfaces.snorm_normal_map(53, 101)), ("boundary_128", ref.boundary_heavy_snorm())):
        out[name + ".input"] = img
        out[name + ".bc4_snorm"] = ref.encode(1, img)
        out[name + ".bc5_snorm"] = ref.encode(2, img)
    return out


def main():
    new = build()
    if "--check" in sys.argv[1:]:
        old = dict(np.load(PATH))
        bad = [k for k in new if k not in old or not np.array_equal(old[k], new[k])] + [k for k in old if k not in new]
        print("golden_bc45_snorm.npz:", "up to date" if not bad else f"differs in {bad}")
        return 1 if bad else 0
    np.savez_compressed(PATH, **new)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
