"""The argument behind the pair route of the RGB bounded order (csrc/bc7.hip, PAIRS), pinned on the CPU with what the oracle exports and
independently of the kernels.  Per block: inc = what modes 1/3 have to get strictly below (the `slow` encode without them, + 1 when a mode
4/5/6 holds the block: bc7_finish_all<3>'s rule), LB = two_subset_bound of the 64 shapes, P1 = {s : LB(s) < inc - 0.5}.  Per mode, the
reference refines s* = the ordered argmin (fast error, then rank key) over all 64 shapes (kernel.ispc:1299-1363).  With E1 the ordered
minimum over P1 and P2 = {s outside P1 : LB(s) <= E1} where E1 >= inc:
  (1) the ordered argmin over P1 + P2 lies in P1 exactly when s* does, and then it is s*;
  (1') what the kernels use of it: E1 < inc alone already makes the P1 winner s* (P2 is empty), and a mode whose P1 is empty has s* outside;
  (2) where (1) says neither mode can act, the full `slow` encode equals the encode without modes 1/3."""
import ctypes as C

import numpy as np
import pytest

from test_bc7_bound import sample_images, planar_blocks, lib, bounds_of
from oracle import pyoracle


def _winner_mode(data):
    b0 = int(data[0]) & 0xff
    return (b0 & -b0).bit_length() - 1


def _ordered_argmin(err, key, members):
    best = None
    for s in members:
        c = (float(err[s]), int(key[s]))
        if best is None or c < best[0]:
            best = (c, s)
    return best                                   # ((error, key), shape) or None


def rule_of_block(L, block, full, no13):
    """-> inc, per mode (s_star, rule winner or None when it is outside P1, |P1|, |P2|, E1), and the two encodes' words"""
    data = (C.c_uint32 * 4)()
    e = C.c_float()
    L.oracle_bc7_block(block.ctypes.data, C.byref(no13), data, C.byref(e))
    without = tuple(data)
    inc = int(e.value) + (1 if _winner_mode(data) in (4, 5, 6) else 0)
    L.oracle_bc7_block(block.ctypes.data, C.byref(full), data, C.byref(e))
    lb = bounds_of(L, block)
    p1 = [s for s in range(64) if lb[s] < inc - 0.5]
    err = np.zeros(64, np.float32)
    key = np.zeros(64, np.int32)
    modes = {}
    for mode in (1, 3):
        L.oracle_bc7_part_fast_errors(block.ctypes.data, mode, err.ctypes.data, key.ctypes.data)
        star = _ordered_argmin(err, key, range(64))[1]
        w1 = _ordered_argmin(err, key, p1)
        p2 = []
        if w1 is not None and w1[0][0] >= inc:
            p2 = [s for s in range(64) if s not in p1 and lb[s] <= w1[0][0]]
        w = _ordered_argmin(err, key, p1 + p2)
        winner = w[1] if (w is not None and w[1] in p1) else None
        modes[mode] = (star, winner, len(p1), len(p2), None if w1 is None else w1[0][0], None if w1 is None else w1[1])
    return inc, p1, modes, without, tuple(data)


@pytest.mark.parametrize("name,img", list(sample_images()), ids=[n for n, _ in sample_images()])
def test_pair_rule_names_the_references_shape_or_says_outside(name, img):
    L = lib()
    L.oracle_bc7_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.oracle_bc7_block.restype = None
    full = pyoracle.bc7_profile("slow")
    no13 = pyoracle.bc7_profile("slow")
    no13.fastSkipTreshold_mode1 = 0
    no13.fastSkipTreshold_mode3 = 0
    blocks = planar_blocks(img)
    inside = outside = quiet = early = listed = 0
    for b in range(blocks.shape[0]):
        inc, p1, modes, without, with13 = rule_of_block(L, blocks[b], full, no13)
        listed += len(p1) > 0
        for mode, (star, winner, n1, n2, e1, s1) in modes.items():
            # (1)
            assert (winner is not None) == (star in p1), (name, b, mode, star, winner, n1, n2)
            if winner is not None:
                assert winner == star, (name, b, mode, star, winner)
                inside += 1
            else:
                outside += 1
            # (1')
            if e1 is not None and e1 < inc:
                assert s1 == star, (name, b, mode, s1, star, e1, inc)
                early += 1
            if n1 == 0:
                assert star not in p1
        # (2)
        if all(m[1] is None for m in modes.values()):
            assert with13 == without, (name, b, inc)
            quiet += 1
    print(f"{name}: {blocks.shape[0]} blocks, per (block, mode): s* inside P1 {inside}, outside {outside}, decided by E1 < inc {early}; "
          f"blocks where neither mode can act {quiet}, blocks with a non-empty P1 {listed}")
    # not vacuous: both sides of (1) occur on every image some block of which the bound lists at all.  One sample has none (the 64 x 64
    # crop of colors260k: smooth ramps the other modes encode so well that no shape's bound is below any block's incumbent -- 0 of 256
    # blocks listed): there the rule must say "outside" for every block and mode, which is the second side alone
    assert outside > 0 and quiet > 0, (name, outside, quiet)
    if listed:
        assert inside > 0, (name, inside, outside, listed)
    else:
        assert name == "colors260k" and outside == 2 * blocks.shape[0] and quiet == blocks.shape[0], (name, outside, quiet)
