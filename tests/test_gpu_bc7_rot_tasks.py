"""Modes 4/5 of the RGB bounded order as tasks over the (block, rotation) pairs a bound leaves (csrc/bc7.hip: bc7_finish_all<9>,
bc7_rot_tasks, bc7_finish_all<10>): `slow` with the route on (default), off (ITW_BC7_ROT_TASKS=0: bc7_finish_all<3>, all nine candidates
of every block inline), and on together with the pair route off / forced into its overflow route emits the oracle's bytes.  The switches
are read at every call, so one process compares the routes.  The device's rotation bound (itwTestBc7RotationBounds) is held against the
exact value in float64: never above it, and not uselessly below."""
import os
import sys

import numpy as np
import pytest

from conftest import first_mismatch
from test_bc7_bound import adversarial_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bc7_rotation_survival as study  # noqa: E402

pytestmark = pytest.mark.gpu

SWITCHES = ("ITW_BC7_ROT_TASKS", "ITW_BC7_PAIRS", "ITW_BC7_PAIR_CAP")
ROUTES = {"rot_tasks": {}, "inline": {"ITW_BC7_ROT_TASKS": "0"}, "rot_tasks_full_scan": {"ITW_BC7_PAIRS": "0"}, "rot_tasks_overflow": {"ITW_BC7_PAIR_CAP": "1"}}


@pytest.fixture
def deep(itw):
    itw.set_bc7_path("deep")            # the fused shape whatever the size (small surfaces: its one-band route)
    yield
    itw.set_bc7_path("auto")


def _encode(itw, gpu, img, env, pilot, settings="slow", out=None):
    import torch
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    itw.set_bc7_pilot(pilot)
    try:
        src = img if hasattr(img, "data_ptr") else torch.from_numpy(img).to(gpu)
        got = itw.compress("bc7", src, settings, out=out) if out is not None else itw.compress("bc7", src, settings)
        torch.cuda.synchronize()
        return got.cpu().numpy()
    finally:
        itw.set_bc7_pilot(None)
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _check(itw, gpu, img, want, settings="slow", what=""):
    """every route under the pilot's own verdict and with the bounded order forced (100): the oracle's bytes, hence each other's"""
    for pilot in (None, 100):
        for route, env in ROUTES.items():
            got = _encode(itw, gpu, img, env, pilot, settings)
            assert first_mismatch(got, want, 16) is None, (what, route, pilot, first_mismatch(got, want, 16))


def _tiled(oracle, base, ry, rx):
    """`base` (sides multiples of 4) repeated ry x rx times and the oracle's blocks of it: the oracle encodes the base once"""
    h, w = base.shape[0] // 4 * 4, base.shape[1] // 4 * 4
    base = np.ascontiguousarray(base[:h, :w])
    want = oracle.encode_mt("bc7", base, "slow").reshape(h // 4, w // 4, 16)
    return np.ascontiguousarray(np.tile(base, (ry, rx, 1))), np.ascontiguousarray(np.tile(want, (ry, rx, 1))).reshape(-1)


@pytest.fixture(scope="module")
def mixed(golden_inputs, oracle):
    """noise over smooth fields, a photograph, few-level content and two-colour blocks (test_gpu_bc7_bound._mixed_content): 23 x 25 = 575
    blocks (one band, every list ends inside a wave) and 129 x 151 blocks (two bands, a partial last chunk); encoded by the oracle once"""
    from test_gpu_bc7_bound import _mixed_content
    out = {}
    for h, w in ((92, 100), (516, 604)):
        img = _mixed_content(golden_inputs, h, w)
        out[(h, w)] = (img, oracle.encode_mt("bc7", img, "slow"))
    return out


@pytest.mark.parametrize("h,w", [(92, 100), (516, 604)], ids=["one_band_575_blocks", "two_bands_partial_chunk"])
def test_mixed_content_at_odd_sizes(itw, gpu, deep, mixed, h, w):
    img, want = mixed[(h, w)]
    assert (img.shape[0] // 4) * (img.shape[1] // 4) % 64 != 0
    _check(itw, gpu, img, want)


def test_adversarial_blocks_one_band(itw, gpu, oracle, deep):
    """flat blocks have e02 = 0: they reach no rotation list; two-level and collinear blocks tie massively between candidates: the merged
    word has to keep the reference's order (mode 4 before mode 5, the lower rotation first)"""
    img = adversarial_blocks(np.random.default_rng(5))
    assert img.shape[0] * img.shape[1] // 16 < 32 * 256
    _check(itw, gpu, img, oracle.encode_mt("bc7", img, "slow"))


def test_adversarial_blocks_two_bands(itw, gpu, oracle, deep):
    img, want = _tiled(oracle, adversarial_blocks(np.random.default_rng(20260927)), 33, 1)
    assert img.shape[0] * img.shape[1] // 16 >= 32 * 256
    _check(itw, gpu, img, want)


def test_pure_noise_every_rotation_survives(itw, gpu, oracle, deep):
    """noise of +-2 about one colour: every plane's residual stays within the rounding slack (bound 0) while the coarse endpoints of
    modes 0/2 leave an error of 70 and more -- all three lists hold every block.  (Noise over the whole range does the opposite: three
    subsets beat one line in a plane and most rotations are excluded.)"""
    rng = np.random.default_rng(9)
    base = np.clip(rng.integers(3, 253, (1, 1, 4)) + rng.integers(-2, 3, (32, 36, 4)), 0, 255).astype(np.uint8)
    base[..., 3] = 255
    blk = study.blocks_of(base)
    sv = study.survivors(study.rotation_bounds_f32(blk), study.errors_02(base))
    assert sv.all()
    img, want = _tiled(oracle, base, 12, 11)                     # 96 x 99 blocks: two bands, lists of 9504 = 148.5 waves
    assert img.shape[0] * img.shape[1] // 16 >= 32 * 256 and (img.shape[0] * img.shape[1] // 16) % 64 != 0
    _check(itw, gpu, img, want)


def test_flat_surface_all_three_lists_empty(itw, gpu, oracle, deep):
    base = np.empty((8, 8, 4), np.uint8)
    base[...] = (37, 120, 201, 255)
    img, want = _tiled(oracle, base, 48, 51)                     # 96 x 102 blocks: two bands
    assert img.shape[0] * img.shape[1] // 16 >= 32 * 256
    _check(itw, gpu, img, want)


VARIANTS = [("channel0", 0), ("channel0", 1), ("channel0", 2), ("no_modes_45", None), ("channel_iters", 0), ("channel_iters", 2), ("iters_45", 0), ("iters_45", 2)]


@pytest.mark.parametrize("field,value", VARIANTS, ids=[f"{f}-{v}" for f, v in VARIANTS])
def test_custom_structs(itw, gpu, oracle, deep, mixed, field, value):
    """first rotation 0 / 1 / 2 (no tasks below it), the group off (no tasks at all), and the candidates' refinement counts"""
    img = mixed[(92, 100)][0]
    s, o = itw.bc7_profile("slow"), oracle.bc7_profile("slow")
    for t in (s, o):
        if field == "channel0":
            t.mode45_channel0 = value
        if field == "no_modes_45":
            t.mode_selection[2] = 0
        if field == "channel_iters":
            t.refineIterations_channel = value
        if field == "iters_45":
            t.refineIterations[4] = value
            t.refineIterations[5] = value
    want = oracle.encode_mt("bc7", img, o)
    _check(itw, gpu, img, want, s, (field, value))


def test_device_bound_against_the_exact_bound(itw, gpu, golden_inputs, mixed):
    import torch
    from itw_amd import surfaces
    imgs = [adversarial_blocks(np.random.default_rng(20260927)), mixed[(92, 100)][0],
            np.ascontiguousarray(surfaces.ldr_smooth(4096, 4096, surfaces.SEED)[1024:1152, 2048:2176]), np.ascontiguousarray(golden_inputs["baboon"][:128, :128])]
    for k, img in enumerate(imgs):
        got = itw.bc7_rotation_bounds(torch.from_numpy(img).to(gpu)).cpu().numpy()
        blk = study.blocks_of(img)
        exact = study.rotation_bounds_f64(blk)
        assert got.shape == exact.shape
        over = got.astype(np.float64) > exact
        assert not over.any(), (k, np.argwhere(over)[:4], got[over][:4], exact[over][:4])
        loose = got.astype(np.float64) < exact * (1 - 1e-3) - 1.0
        assert not loose.any(), (k, np.argwhere(loose)[:4], got[loose][:4], exact[loose][:4])
        # the numpy restatement rounds every operation once where the device's rcp / sqrt are good to 1 ulp: a few ulps of 1 in the scaled
        # residual, times the trace (below 2^25) / 16 -- at most 0.5 in the bound, far less on ordinary blocks
        assert np.allclose(got, study.rotation_bounds_f32(blk), rtol=1e-4, atol=0.5)


def test_route_writes_exactly_its_output(itw, gpu, deep, mixed):
    """guard bands around the destination and the source (tests/_guarded.py) with the route on, two bands and a partial chunk: the lists,
    payload slots and merged words live in the library's own workspace, whose capacities are the band's block count"""
    from _guarded import frozen, guarded
    img, want = mixed[(516, 604)]
    src = frozen(img, row_pad=48, device=gpu)
    out = guarded(want.size, device=gpu)
    for rnd in (1, 2):
        out.refill()
        _encode(itw, gpu, src.view, {}, 100, out=out.view)
        m = first_mismatch(out.host(), want, 16)
        assert m is None, (rnd, m)
        out.check(f"rot tasks, call {rnd}, destination")
        src.check(f"rot tasks, call {rnd}, source")
