"""bc7_bound_list (csrc/bc7.hip): the tail of the RGB bounded order's rotation-task route -- the 64 two-subset bounds, the list of modes 1/3, the
pairs bucketed by shape, the heavy blocks, the compact texels -- runs in a kernel of its own behind bc7_finish_all<10>, which now stops at the
incumbent it leaves in inc_err; bc7_finish_all<3> and <5> call the same device function (bounded_list_tail) in place.  Byte equality with the
oracle is the whole contract, and which blocks are listed, paired and deferred does not depend on which kernel runs the bounds: every call's
device counters (itwTestBc7CallCounters) are held against those the PARENT commit's hooks build gave for the same surface and switches
(tests/golden/bc7_bound_kernel_parent_counters.json, tools/bc7_bound_kernel_counters.py).

Geometries (columns x rows), each for a way the kernel can go wrong:
    604 x 516   76.1 chunks of 256 blocks, two bands: a ragged last workgroup whose idle lanes must still reach the claim's two barriers
    128 x 96    3 chunks: the single-band route, no pilot
    12 x 8      6 blocks: one workgroup, 250 idle lanes
Contents (tools/bc7_bound_kernel_counters.py), each asserting on the oracle's stream or the counters what it is there for:
    smooth      the bench surface's generator: blocks are listed, pairs are made, some are deferred (604 x 516 of it defers 43)
    ramp_half   left a noiseless colour ramp, right the generator: mode 6 runs and wins in lanes of waves whose other lanes are the generator's
    channel     blue varies independently of red and green: modes 4/5 win, so bc7_finish_all<10> admitted a candidate and inc took its + 1
    baboon      the golden photograph tiled, the pilot forced to each verdict: heavy blocks on the second list; under the other verdict the
                gated kernel returns at once
Every case runs under ITW_BC7_ROT_TASKS 1 / 0 x ITW_BC7_PAIRS 1 / 0 (PAIRS=0: the per-wave append with its early exit and bail; ROT_TASKS=0:
bc7_finish_all<3> calls the shared tail in place) and with a bucket capacity of one pair (overflow), each twice: the lists' order is a race between
workgroups and must not reach the output."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import first_mismatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bc7_bound_kernel_counters as bk  # noqa: E402
import bc7_waits_counters as waits  # noqa: E402

pytestmark = pytest.mark.gpu

REPEATS = ("first", "again")
ROT_LISTS = ("rot00", "rot01", "rot02", "rot10", "rot11", "rot12")


@pytest.fixture(scope="module")
def parent_counters():
    with open(os.path.join(ROOT, "tests", "golden", "bc7_bound_kernel_parent_counters.json")) as f:
        return json.load(f)["counters"]


@pytest.fixture(scope="module")
def hooks(itw):
    """the hooks build, deep path (the fused shape whatever the size), its device counters armed"""
    T = itw.test_lib()
    T.itwSetBc7Path(itw.abi.BC7_PATH["deep"])
    T.itwTestBc7CallCountersArm(1)
    yield T
    T.itwTestBc7CallCountersArm(0)
    T.itwSetBc7Pilot(-2)
    T.itwSetBc7Path(itw.abi.BC7_PATH["auto"])


@pytest.fixture(scope="module")
def references(oracle, golden_inputs):
    """(content, rows, columns) -> (surface, the oracle's blocks); the tiled photograph is encoded once"""
    bab = waits.baboon_base(golden_inputs)
    bab_want = oracle.encode_mt("bc7", bab, "slow")
    out = {}
    for h, w in bk.SIZES:
        for name in bk.CONTENTS:
            img = bk.surface(name, golden_inputs, h, w)
            want = waits.tile_blocks_to(bab_want, bab.shape, h, w) if name == "baboon" else oracle.encode_mt("bc7", img, "slow")
            out[(name, h, w)] = (img, want)
    return out


def longest_run(flags):
    best = run = 0
    for f in flags:
        run = run + 1 if f else 0
        best = max(best, run)
    return best


CASES = [(name, h, w) for h, w in bk.SIZES for name in bk.CONTENTS]


@pytest.mark.parametrize("name,h,w", CASES, ids=[f"{n}-{w}x{h}" for n, h, w in CASES])
def test_same_bytes_and_same_counts_on_every_route(itw, gpu, hooks, references, parent_counters, name, h, w):
    import torch
    img, want = references[(name, h, w)]
    nblocks = (h // 4) * (w // 4)
    big = nblocks >= 32 * 256                                            # two bands and a pilot
    # what the content is there for, on the oracle's stream
    modes = bk.block_modes(want)
    if name == "ramp_half":
        assert (modes == 6).any(), np.bincount(modes, minlength=8)
        assert longest_run(modes == 6) < 64, longest_run(modes == 6)     # no wave is all mode 6: lanes where it wins beside lanes where it does not run
        assert (modes[np.arange(nblocks) % (w // 4) >= bk.left_columns(w) // 4] != 6).all()
    if name == "channel":
        assert ((modes == 4) | (modes == 5)).any(), np.bincount(modes, minlength=8)
    src = torch.from_numpy(img).to(gpu)
    seen = {}
    for pilot in bk.pilots(name):
        for route, env in bk.ROUTES:
            parent = parent_counters[bk.key(name, h, w, pilot, route)]
            assert sorted(parent) == sorted(itw.abi.BC7_CALL_COUNTERS), parent      # the record holds every count: two calls of the parent agreed on all
            for gname in REPEATS:
                what = (name, h, w, pilot, route, gname)
                got, ctr = bk.encode(itw, hooks, gpu, src, env, pilot)
                m = first_mismatch(got, want, 16)
                assert m is None, (what, m)
                mine = {k: ctr[k] for k in parent}
                assert mine == parent, (what, mine, parent)
                if env["ITW_BC7_ROT_TASKS"] == "0":
                    assert not any(ctr[k] for k in ROT_LISTS), (what, ctr)
                if env["ITW_BC7_PAIRS"] == "0":
                    assert ctr["pairs0"] == ctr["pairs1"] == 0, (what, ctr)
                seen[(pilot, route)] = ctr
    # ... and on the counters (both calls of a route agree with the parent's record, hence with each other)
    c = seen[(100, "rot1-pairs1")]
    cap1 = seen[(100, "rot1-cap1")]
    assert c["listed0"] > 0 and c["pairs0"] > 0, c                                # at every geometry the new kernel listed blocks and made pairs
    if name == "smooth" and big:
        assert c["pilot_flag"] == 1 and c["listed0"] > 0 and c["listed1"] > 0 and c["pairs0"] > 0 and c["pairs1"] > 0, c
        assert c["overflow0"] == c["overflow1"] == 0 and c["redo0"] + c["redo1"] == 43, c
        assert seen[(100, "rot0-pairs1")]["redo0"] + seen[(100, "rot0-pairs1")]["redo1"] == 43
        assert seen[(100, "rot1-pairs0")]["listed0"] >= c["listed0"], seen          # the bail lists blocks the bounds alone would not
    if name == "smooth" and nblocks >= 256:
        assert cap1["overflow0"] and cap1["redo0"] == cap1["listed0"] == c["listed0"] > 0, cap1    # every listed block takes the band's redo
    if name == "ramp_half" and big:
        assert c["listed0"] > 0 and c["listed1"] > 0 and c["pairs0"] > 0 and c["pairs1"] > 0, c
    if name == "channel" and big:
        assert all(c[k] > 0 for k in ROT_LISTS), c                                # candidates for bc7_finish_all<10> to admit
    if name == "baboon" and big:
        off = seen[(0, "rot1-pairs1")]
        assert off["pilot_flag"] == 0 and not any(off[k] for k in ("listed0", "listed1", "pairs0", "pairs1", "redo0", "redo1")), off   # returned at once
        assert c["pilot_flag"] == 1 and c["listed0"] > 0 and c["listed1"] > 0, c
        assert c["redo0"] > c["listed0"] // 4 and c["redo1"] > c["listed1"] // 4 and c["overflow0"] == c["overflow1"] == 0, c     # heavy blocks
        assert cap1["overflow0"] and cap1["overflow1"] and (cap1["redo0"], cap1["redo1"]) == (c["listed0"], c["listed1"]), cap1
