"""How many (block, shape) pairs of the RGB bounded order's list scan the bound leaves (csrc/bc7.hip, PAIRS) -- on the CPU, with the
oracle's own functions: oracle_bc7_block without modes 1/3 for the incumbent `inc` (+ 1 when a mode 4/5/6 holds the block, as
bc7_finish_all<3> does), oracle_bc7_two_subset_bound for LB, oracle_bc7_part_fast_errors for the fast errors and rank keys.
  listed        blocks with some LB(s) < inc - 0.5 (what finish<3> lists; the full list scan fits 64 shapes of each, both modes)
  P1            the shapes of a listed block with LB(s) < inc - 0.5: what bc7_finish_all<3> leaves as pairs (pass 1)
  P2            per mode, where the P1 winner's fast error E1 >= inc: shapes outside P1 with LB(s) <= E1 (pass 2 of a two-pass scheme)
  open          (listed block, mode) with E1 >= inc: the kernels refine the P1 winner anyway and send the block to the full scan only if
                that refinement gets below the incumbent (the count of those comes from the GPU: ITW_BC7_PILOT_DEBUG=1)
  heavy         listed blocks with more than 32 shapes in P1: straight to the full scan
usage: python tools/bc7_pair_survival.py [blocks of the bench surface, default 3000] [blocks per photograph, default 2000] > profiles/bc7_pair_survival.txt"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
from oracle import pyoracle  # noqa: E402
from itw_amd import surfaces  # noqa: E402


def planar_blocks(img):
    h, w = img.shape[0] // 4 * 4, img.shape[1] // 4 * 4
    return np.ascontiguousarray(img[:h, :w].astype(np.float32).reshape(h // 4, 4, w // 4, 4, 4).transpose(0, 2, 4, 1, 3).reshape(-1, 64))


def study(L, name, blocks):
    no13 = pyoracle.bc7_profile("slow")
    no13.fastSkipTreshold_mode1 = 0
    no13.fastSkipTreshold_mode3 = 0
    data = (C.c_uint32 * 4)()
    e = C.c_float()
    err = np.zeros(64, np.float32)
    key = np.zeros(64, np.int32)
    n1, n2, opened, heavy = [], {1: 0, 3: 0}, {1: 0, 3: 0}, 0
    for blk in blocks:
        L.oracle_bc7_block(blk.ctypes.data, C.byref(no13), data, C.byref(e))
        b0 = int(data[0]) & 0xff
        mode = (b0 & -b0).bit_length() - 1
        inc = int(e.value) + (1 if mode in (4, 5, 6) else 0)
        lb = np.array([L.oracle_bc7_two_subset_bound(blk.ctypes.data, p) for p in range(64)], dtype=np.float64)
        p1 = lb < inc - 0.5
        if not p1.any():
            continue
        n1.append(int(p1.sum()))
        heavy += int(p1.sum()) > 32
        for m in (1, 3):
            L.oracle_bc7_part_fast_errors(blk.ctypes.data, m, err.ctypes.data, key.ctypes.data)
            e1 = float(err[p1].min())
            if e1 >= inc:
                opened[m] += 1
                n2[m] += int((~p1 & (lb <= e1)).sum())
    listed = len(n1)
    n1 = np.array(n1 if n1 else [0])
    light = n1[n1 <= 32]
    left = (n1.sum() + 0.5 * (n2[1] + n2[3])) / (64.0 * max(listed, 1))
    kernels = (light.sum() + 64.0 * heavy) / (64.0 * max(listed, 1))
    print(f"{name:16s} {len(blocks):6d} {listed / len(blocks):7.3f} {n1.mean():8.1f} {int(np.median(n1)):6d} {int(np.percentile(n1, 90)):5d} "
          f"{n2[1] / max(listed, 1):7.1f} {n2[3] / max(listed, 1):6.1f} {left:9.3f} {opened[1] / max(listed, 1):8.3f} {opened[3] / max(listed, 1):6.3f} "
          f"{heavy / max(listed, 1):7.3f} {kernels:9.3f}")


def main():
    nb = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
    npic = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
    L = pyoracle.lib()
    L.oracle_bc7_two_subset_bound.argtypes = [C.c_void_p, C.c_int]
    L.oracle_bc7_two_subset_bound.restype = C.c_float
    L.oracle_bc7_part_fast_errors.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.oracle_bc7_part_fast_errors.restype = None
    L.oracle_bc7_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.oracle_bc7_block.restype = None
    rng = np.random.default_rng(20261016)
    z = np.load(os.path.join(ROOT, "tests", "golden", "inputs.npz"))
    print("# tools/bc7_pair_survival.py: `slow`, random blocks of each surface (seed 20261016); per listed block unless said otherwise")
    print("# left = (|P1| + (|P2(mode 1)| + |P2(mode 3)|) / 2) / 64: shape evaluations of a two-pass scheme against the full list scan's")
    print("# kernels = what bc7_finish_all<3> sends on: |P1| of the blocks with |P1| <= 32 as pairs, 64 shapes of the heavier ones, / 64")
    print(f"{'content':16s} {'blocks':>6s} {'listed':>7s} {'P1 mean':>8s} {'median':>6s} {'p90':>5s} {'P2 m1':>7s} {'P2 m3':>6s} {'left':>9s} {'open m1':>8s} {'m3':>6s} {'heavy':>7s} {'kernels':>9s}")
    for name, img, n in (("bench surface I3", surfaces.ldr_smooth(4096, 4096, surfaces.SEED), nb), ("baboon", z["baboon"], npic), ("monkey", z["monkey"], npic)):
        blocks = planar_blocks(img)
        pick = rng.choice(blocks.shape[0], min(n, blocks.shape[0]), replace=False)
        study(L, name, blocks[pick])


if __name__ == "__main__":
    main()
