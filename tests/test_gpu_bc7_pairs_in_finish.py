"""bc7_finish_all<3> leaves the pairs itself (csrc/bc7.hip, PAIRS: the bound loop keeps a bit per shape, no early exit and no bail while
the pair route is on; the builder kernel behind it is gone).  Two things that change with it, pinned to the oracle under every route of
tests/test_gpu_bc7_pairs.py:
  * content that makes whole waves hit the bail rule (BOUND_BAIL_AFTER / BOUND_BAIL_LANES) inside a call the pilot gives to the bounded
    order: with ITW_BC7_PAIRS=0 those waves bail as ever, with the route on they bound all 64 shapes, with ITW_BC7_PAIR_CAP=1 their
    buckets overflow;
  * blocks with exactly 32 and exactly 33 surviving shapes, on either side of PAIR_MAX_PER_BLOCK.  Both sides emit the same bytes by design,
    so the bytes show that both routes work, not where the boundary lies; the boundary is pinned by the band counters the library prints under
    ITW_BC7_PILOT_DEBUG=1: the buckets must hold exactly the survivors of the blocks with 1 .. 32 of them."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_bc7_pairs import ROUTES, _check, _tiled

pytestmark = pytest.mark.gpu


@pytest.fixture
def deep(itw):
    itw.set_bc7_path("deep")
    yield
    itw.set_bc7_path("auto")


def test_photograph_chunks_inside_bench_content(itw, gpu, oracle, deep, golden_inputs):
    """128 x 256 blocks: a chunk is one block row, a band's stripe eight of them.  Sixteen whole rows of photograph (both bands), and
    stretches of 128 blocks of it in the middle of eight further rows (waves 1 and 2 of those chunks; waves 0 and 3 stay bench content):
    a photograph lists ~94 % of its blocks, so its waves pass 40 listed lanes within the first four shapes"""
    from itw_amd import surfaces
    assert set(ROUTES) >= {"pairs", "full_scan", "overflow"}
    img = surfaces.ldr_smooth(512, 1024, seed=surfaces.SEED + 5).copy()
    photo = np.tile(golden_inputs["baboon"], (2, 4, 1))
    assert photo.shape == img.shape
    img[64:128] = photo[64:128]
    img[200:232, 256:768] = photo[200:232, 256:768]
    img[..., 3] = 255
    img = np.ascontiguousarray(img)
    assert img.shape[0] * img.shape[1] // 16 >= 32 * 256          # two bands, the pilot runs
    _check(itw, gpu, img, oracle.encode_mt("bc7", img, "slow"), pilots=(100, None))


def _survivors(itw, gpu, oracle, img):
    """per block of `img`: how many two-subset shapes the DEVICE's bound leaves below the incumbent of modes 1/3 -- the oracle's error without
    those modes, + 1 where a mode 4/5/6 holds the block (bc7_finish_all<3>'s rule; tools/bc7_pair_survival.py)"""
    import torch
    from test_bc7_bound import planar_blocks
    L = oracle.lib()
    L.oracle_bc7_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.oracle_bc7_block.restype = None
    no13 = oracle.bc7_profile("slow")
    no13.fastSkipTreshold_mode1 = 0
    no13.fastSkipTreshold_mode3 = 0
    lb = itw.bc7_two_subset_bounds(torch.from_numpy(img).to(gpu)).cpu().numpy()
    blocks = planar_blocks(img)
    data = (C.c_uint32 * 4)()
    e = C.c_float()
    out = np.zeros(blocks.shape[0], np.int32)
    for b in range(blocks.shape[0]):
        L.oracle_bc7_block(blocks[b].ctypes.data, C.byref(no13), data, C.byref(e))
        b0 = int(data[0]) & 0xff
        mode = (b0 & -b0).bit_length() - 1
        inc = int(e.value) + (1 if mode in (4, 5, 6) else 0)
        out[b] = int((~(lb[b] >= np.float32(inc) - np.float32(0.5))).sum())
    return out


_COUNTERS_CHILD = """
import sys
import numpy as np, torch
import itw_amd
itw_amd.set_bc7_path("deep")
itw_amd.set_bc7_pilot(100)
img = np.load(sys.argv[1])
itw_amd.compress("bc7", torch.from_numpy(img).to(torch.device("cuda:0")), "slow")
torch.cuda.synchronize()
"""


def _pair_counters(img, tmp_path):
    """(pairs in the buckets, blocks on the second lists), both bands, of one `slow` call in the bounded order: a child process, because the
    library reads ITW_BC7_PILOT_DEBUG once"""
    path = str(tmp_path / "surface.npy")
    np.save(path, img)
    env = dict(os.environ, ITW_BC7_PILOT_DEBUG="1")
    for k in ("ITW_BC7_PAIRS", "ITW_BC7_PAIR_CAP", "ITW_BC7_BANDS", "ITW_BC7_PILOT_THR"):
        env.pop(k, None)
    env["PYTHONPATH"] = os.pathsep.join(p for p in sys.path if p)
    r = subprocess.run([sys.executable, "-c", _COUNTERS_CHILD, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = re.findall(r"bc7 pairs: band (\d): (\d+) pairs, .* deferred to the full scan (\d+)", r.stderr)
    assert sorted(b for b, _, _ in rows) == ["0", "1"], r.stderr[-2000:]
    return sum(int(p) for _, p, _ in rows), sum(int(d) for _, _, d in rows)


def test_blocks_with_exactly_32_and_33_surviving_shapes(itw, gpu, oracle, deep, golden_inputs, tmp_path):
    """found in the golden photograph with the bound test hook, not constructed: every such block of baboon (and its neighbours in the count,
    30 .. 35), gathered into one strip, repeated to two bands' worth of chunks.  Bytes on every route; then the counters: the buckets hold
    the survivors of the blocks with at most 32 of them and nothing of the others, which the second lists hold at least"""
    bab = np.ascontiguousarray(golden_inputs["baboon"])
    bab[..., 3] = 255
    n = _survivors(itw, gpu, oracle, bab)
    assert (n == 32).any() and (n == 33).any(), ("no block with exactly 32 / 33 survivors in baboon", int((n == 32).sum()), int((n == 33).sum()))
    pick = np.nonzero((n >= 30) & (n <= 35))[0]
    bx = bab.shape[1] // 4
    k = (len(pick) // 64) * 64 or len(pick)                       # whole waves of them where there are enough
    strip = np.concatenate([bab[(i // bx) * 4:(i // bx) * 4 + 4, (i % bx) * 4:(i % bx) * 4 + 4] for i in pick[:k]], axis=1)
    again = _survivors(itw, gpu, oracle, np.ascontiguousarray(strip))
    assert (again == n[pick[:k]]).all() and (again == 32).any() and (again == 33).any()
    reps = -(-32 * 256 // k)
    img, want = _tiled(oracle, strip, reps, 1)
    assert img.shape[0] * img.shape[1] // 16 >= 32 * 256
    _check(itw, gpu, img, want, pilots=(100, None))
    pairs, deferred = _pair_counters(img, tmp_path)
    light, heavy = again[again <= 32], again[again > 32]
    assert pairs == int(light.sum()) * reps, (pairs, int(light.sum()) * reps, int(again.sum()) * reps)
    assert deferred >= len(heavy) * reps and len(heavy) > 0, (deferred, len(heavy) * reps)
