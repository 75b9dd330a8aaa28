"""Modes 4/5 of the RGB bounded order run only for the (block, rotation) pairs whose bound is still below the error modes 0/2 left
(csrc/bc7.hip bc7_rot_tasks, csrc/bc7_exact.hpp rotation_bound).  That rests on ONE property: no mode 4/5 candidate of a rotation gets
below that rotation's bound.  CPU side: the float32 bound as the device computes it, restated in numpy (tools/bc7_rotation_survival.py),
against the oracle -- wherever modes 4/5 take a block from modes 0/2, the winner's rotation must be among the survivors -- and against the
exact value in float64, which it must never exceed.  The device function is compared with both in tests/test_gpu_bc7_rot_tasks.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import pyoracle  # noqa: E402
from itw_amd import surfaces  # noqa: E402
import bc7_rotation_survival as study  # noqa: E402
from test_bc7_bound import adversarial_blocks  # noqa: E402


def contents():
    z = np.load(os.path.join(ROOT, "tests", "golden", "inputs.npz"))
    return {"adversarial": adversarial_blocks(np.random.default_rng(20260927)),
            "bench_surface": np.ascontiguousarray(surfaces.ldr_smooth(4096, 4096, surfaces.SEED)[1024:1152, 2048:2176]),
            "baboon": np.ascontiguousarray(z["baboon"][:128, :128])}


@pytest.fixture(scope="module", params=["adversarial", "bench_surface", "baboon"])
def content(request):
    img = contents()[request.param]
    blk = study.blocks_of(img)
    return img, blk, study.rotation_bounds_f32(blk), study.rotation_bounds_f64(blk)


def test_float32_bound_never_exceeds_the_exact_bound(content):
    _, _, b32, b64 = content
    over = b32.astype(np.float64) > b64
    assert not over.any(), (np.argwhere(over)[:4], b32[over][:4], b64[over][:4])
    assert (b32 >= 0).all() and np.isfinite(b32).all()
    # ... and is not uselessly loose: the margins are 1e-5 of the trace and 1e-6 factors
    assert (b32.astype(np.float64) >= b64 * (1 - 1e-3) - 1.0).all()


def test_a_mode_45_winner_has_a_surviving_rotation(content):
    """e02 from the oracle with modes 0/2 alone; the same encode with modes 4/5 added takes a block only with a candidate strictly below
    e02, and that candidate's rotation -- read from the block's bits -- has to be one the bound left"""
    img, _, b32, _ = content
    e02 = study.errors_02(img)
    sv = study.survivors(b32, e02)
    s = pyoracle.bc7_profile("slow")
    s.mode_selection[0], s.mode_selection[1], s.mode_selection[2], s.mode_selection[3] = 1, 0, 1, 0
    h, w = img.shape[0] // 4 * 4, img.shape[1] // 4 * 4
    out = pyoracle.encode("bc7", np.ascontiguousarray(img[:h, :w]), s).reshape(-1, 16)
    first = out[:, 0].astype(np.int64)
    mode = np.log2(first & -first).astype(np.int64)              # the lowest set bit (every block has a mode)
    assert set(np.unique(mode)) <= {0, 2, 4, 5}
    taken = 0
    for b in np.flatnonzero((mode == 4) | (mode == 5)):
        word = int(out[b, 0]) | (int(out[b, 1]) << 8)
        rot_bits = (word >> (5 if mode[b] == 4 else 6)) & 3          # emitted as (rotation + 1) & 3
        assert rot_bits != 0, ("rotation 3 under an RGB profile", b)
        assert sv[b, rot_bits - 1], (b, int(mode[b]), rot_bits - 1, b32[b], int(e02[b]))
        taken += 1
    # flat and collinear blocks have e02 = 0: nothing survives there
    assert not sv[e02 == 0].any()
    print(f"modes 4/5 took {taken} of {out.shape[0]} blocks; {sv.mean():.3f} of the (block, rotation) pairs survive")
