"""The waits taken out of the RGB bounded order's refinement kernels (csrc/bc7.hip): bc7_finish_all<9> claims its three rotation lists once per
workgroup (append_to_rotation_lists: LDS counts, two barriers, one atomic instruction) where every wave made three waited atomics, and
bc7_finish_all<10> / <3> claim the block list's stretch together with the pair buckets'.  Byte equality is the whole contract: `slow` on two
geometries that take the fused two-band route

    604 x 516     76.1 chunks of 256 blocks: a ragged last chunk, idle lanes in the last workgroup of a band that still arrive at the barriers
    2048 x 1024   512 chunks

and three contents (tools/bc7_waits_counters.py) -- the bench surface's generator (604 x 516 of it already defers 43 blocks to the full list
scan), a flat colour, the golden baboon tiled -- under every combination of the pilot's threshold (its own, 0, 100), ITW_BC7_ROT_TASKS 1 / 0 and
ITW_BC7_PAIRS 1 / 0, each twice: every result is the oracle's bytes, hence equal to every other, although the order of the lists differs from
call to call (which workgroup's claim lands first is a race; the merged words' low bits only name a payload slot).  The calls go through the
hooks build, whose device counters (itwTestBc7CallCounters) the test holds against those the PARENT commit's build printed for the same
surfaces (tests/golden/bc7_waits_parent_counters.json: list lengths do not depend on who claims what).  A list that happens to be empty proves
nothing, so each content also asserts what it is there for.

The 2048 x 1024 generator surface is the one reference that is not a tiled base: the oracle encodes its 131 072 blocks once for the module.
(A persistent bc7_finish_all<9> was built and measured with this file -- grids of 3 workgroups, the resident count and more than the band's
chunks -- and dropped: profiles/r10_rejected_experiments.txt.)"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from conftest import first_mismatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bc7_waits_counters as waits  # noqa: E402

pytestmark = pytest.mark.gpu

SWITCHES = ("ITW_BC7_ROT_TASKS", "ITW_BC7_PAIRS", "ITW_BC7_PAIR_CAP")
REPEATS = ("first", "again")


@pytest.fixture(scope="module")
def parent_counters():
    with open(os.path.join(ROOT, "tests", "golden", "bc7_waits_parent_counters.json")) as f:
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
    """(content, rows, columns) -> (surface, the oracle's blocks); tiled contents are encoded once per base"""
    flat_base = np.empty((8, 8, 4), np.uint8)
    flat_base[...] = waits.FLAT
    flat_want = oracle.encode_mt("bc7", flat_base, "slow")
    bab = waits.baboon_base(golden_inputs)
    bab_want = oracle.encode_mt("bc7", bab, "slow")
    out = {}
    for h, w in waits.SIZES:
        smooth = waits.surface("smooth", golden_inputs, h, w)
        out[("smooth", h, w)] = (smooth, oracle.encode_mt("bc7", smooth, "slow"))
        out[("flat", h, w)] = (waits.surface("flat", golden_inputs, h, w), waits.tile_blocks_to(flat_want, flat_base.shape, h, w))
        out[("baboon", h, w)] = (waits.surface("baboon", golden_inputs, h, w), waits.tile_blocks_to(bab_want, bab.shape, h, w))
    return out


def _encode(itw, T, gpu, src, env, pilot, settings=None):
    """one `slow` call through the hooks build -> (blocks, the call's device counters by name)"""
    import torch
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    T.itwSetBc7Pilot(-2 if pilot is None else pilot)
    try:
        h, w = src.shape[:2]
        out = torch.empty((h // 4) * (w // 4) * 16, dtype=torch.uint8, device=gpu)
        st = settings if settings is not None else itw.bc7_profile("slow")
        with torch.cuda.device(gpu):
            T.itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
            surf = itw.RgbaSurface(src.data_ptr(), w, h, src.stride(0))
            T.CompressBlocksBC7(C.byref(surf), out.data_ptr(), C.byref(st))
        torch.cuda.synchronize()
        err = T.itwLastError()
        assert not err, err
        buf = (C.c_int32 * len(itw.abi.BC7_CALL_COUNTERS))()
        T.itwTestBc7CallCounters(buf, len(buf))
        return out.cpu().numpy(), dict(zip(itw.abi.BC7_CALL_COUNTERS, (int(v) for v in buf)))
    finally:
        T.itwSetBc7Pilot(-2)
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


CASES = [(name, h, w) for h, w in waits.SIZES for name in waits.CONTENTS]


@pytest.mark.parametrize("name,h,w", CASES, ids=[f"{n}-{w}x{h}" for n, h, w in CASES])
def test_same_bytes_and_same_counts_on_every_route(itw, gpu, hooks, references, parent_counters, name, h, w):
    import torch
    img, want = references[(name, h, w)]
    nblocks = (h // 4) * (w // 4)
    assert nblocks >= 32 * 256, "the two-band route needs 32 chunks"
    src = torch.from_numpy(img).to(gpu)
    seen = {}
    for pilot in waits.PILOTS:
        parent = parent_counters[waits.key(name, h, w, pilot)]
        for rot in ("1", "0"):
            for pairs in ("1", "0"):
                for gname in REPEATS:
                    what = (name, h, w, pilot, "rot" + rot, "pairs" + pairs, gname)
                    got, ctr = _encode(itw, hooks, gpu, src, {"ITW_BC7_ROT_TASKS": rot, "ITW_BC7_PAIRS": pairs}, pilot)
                    m = first_mismatch(got, want, 16)
                    assert m is None, (what, m)
                    # the pilot's two counts and verdict: the parent's on every route
                    for k in ("pilot_listed", "pilot_sampled", "pilot_flag"):
                        assert ctr[k] == parent[k], (what, k, ctr[k], parent[k])
                    if rot == "1" and pairs == "1":                  # the routes the parent's counters were taken on: every counter
                        assert ctr == parent, (what, ctr, parent)
                        seen[(pilot, gname)] = ctr
                    if rot == "0":
                        assert not any(ctr[k] for k in ("rot00", "rot01", "rot02", "rot10", "rot11", "rot12")), (what, ctr)
                    if pairs == "0":
                        assert ctr["pairs0"] == ctr["pairs1"] == 0, (what, ctr)
    # what each content is there for (both routes on; both calls agree by the assertion above)
    auto, forced = seen[(None, "again")], seen[(100, "again")]
    rot_lists = [forced[k] for k in ("rot00", "rot01", "rot02", "rot10", "rot11", "rot12")]
    if name == "smooth":
        assert auto["pilot_flag"] == 1, auto                        # the bounded order by the pilot's own verdict
        for c in (auto, forced):
            assert all(c[k] > 0 for k in ("rot00", "rot01", "rot02", "rot10", "rot11", "rot12")), c
            assert c["pairs0"] > 0 and c["pairs1"] > 0 and c["listed0"] > 0 and c["listed1"] > 0, c
            assert c["overflow0"] == c["overflow1"] == 0, c
            assert c["redo0"] + c["redo1"] > 0, c                   # blocks deferred to the full list scan behind finish<8>
    if name == "flat":
        # a flat colour has zero variance and the bounds of such a block are not numbers: they exclude nothing, so the parent lists EVERY flat
        # block -- the pilot's own verdict is the reference's order, and under the bounded order every workgroup claims full stretches (256 per
        # list, the ragged workgroup fewer) and every block is deferred.  The claims with a zero total are test_zero_total_claims' below.
        assert auto["pilot_flag"] == 0 and not any(auto[k] for k in ("listed0", "listed1", "rot00", "rot10")), auto
        band = (forced["listed0"], forced["listed1"])
        assert forced["pilot_flag"] == 1 and sum(band) == nblocks and min(band) > 0, forced
        assert rot_lists == [band[0]] * 3 + [band[1]] * 3 and (forced["redo0"], forced["redo1"]) == band and forced["pairs0"] == forced["pairs1"] == 0, forced
    if name == "baboon":
        assert auto["pilot_flag"] == 0 and not any(auto[k] for k in ("listed0", "listed1", "rot00", "rot10")), auto      # the reference's order
        assert seen[(0, "again")]["pilot_flag"] == 0
        assert forced["pilot_flag"] == 1 and all(rot_lists) and forced["listed0"] > 0 and forced["listed1"] > 0, forced
        # photograph content in the bounded order: heavy blocks (more than 32 surviving shapes) go straight to the second list ...
        assert forced["redo0"] > forced["listed0"] // 4 and forced["redo1"] > forced["listed1"] // 4 and forced["overflow0"] == forced["overflow1"] == 0, forced
        # ... and with a bucket capacity of one pair every band overflows: each listed block takes the whole-band redo
        for gname in REPEATS:
            got, ctr = _encode(itw, hooks, gpu, src, {"ITW_BC7_PAIR_CAP": "1"}, 100)
            m = first_mismatch(got, want, 16)
            assert m is None, (name, h, w, "overflow", gname, m)
            assert ctr["overflow0"] and ctr["overflow1"] and (ctr["redo0"], ctr["redo1"]) == (ctr["listed0"], ctr["listed1"]) == (forced["listed0"], forced["listed1"]), (gname, ctr)


def test_zero_total_claims(itw, gpu, hooks, oracle, golden_inputs):
    """modes 4/5 switched off: bc7_finish_all<9> still runs and no lane needs a rotation, so every workgroup's claim has a zero total (no
    atomic); the generator surface at 604 x 516, the bounded order forced"""
    import torch
    h, w = waits.SIZES[0]
    img = waits.surface("smooth", golden_inputs, h, w)
    s, o = itw.bc7_profile("slow"), oracle.bc7_profile("slow")
    s.mode_selection[2] = 0
    o.mode_selection[2] = 0
    want = oracle.encode_mt("bc7", img, o)
    src = torch.from_numpy(img).to(gpu)
    for gname in REPEATS:
        got, ctr = _encode(itw, hooks, gpu, src, {}, 100, settings=s)
        m = first_mismatch(got, want, 16)
        assert m is None, (gname, m)
        assert ctr["pilot_flag"] == 1 and ctr["listed0"] > 0 and not any(ctr[k] for k in ("rot00", "rot01", "rot02", "rot10", "rot11", "rot12")), (gname, ctr)
