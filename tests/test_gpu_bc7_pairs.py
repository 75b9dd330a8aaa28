"""The pair route of the RGB bounded order (csrc/bc7.hip: bc7_pair_build, bc7_pair_scan, bc7_finish_all<8>): `slow` with the route on
(default), off (ITW_BC7_PAIRS=0: the full list scan) and forced into its overflow route (ITW_BC7_PAIR_CAP=1) emits the oracle's bytes.
Both switches are read at every call, so one process compares the routes."""
import os

import numpy as np
import pytest

from conftest import first_mismatch
from test_bc7_bound import adversarial_blocks

pytestmark = pytest.mark.gpu

ROUTES = {"pairs": {}, "full_scan": {"ITW_BC7_PAIRS": "0"}, "overflow": {"ITW_BC7_PAIR_CAP": "1"}, "tight_buckets": {"ITW_BC7_PAIR_CAP": "70"}}


@pytest.fixture
def deep(itw):
    itw.set_bc7_path("deep")            # the fused shape whatever the size (small surfaces: its one-band route)
    yield
    itw.set_bc7_path("auto")


def _encode(itw, gpu, img, env, pilot):
    import torch
    saved = {k: os.environ.get(k) for k in ("ITW_BC7_PAIRS", "ITW_BC7_PAIR_CAP")}
    for k in saved:
        os.environ.pop(k, None)
    os.environ.update(env)
    itw.set_bc7_pilot(pilot)
    try:
        out = itw.compress("bc7", torch.from_numpy(img).to(gpu), "slow")
        torch.cuda.synchronize()
        return out.cpu().numpy()
    finally:
        itw.set_bc7_pilot(None)
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _check(itw, gpu, img, want, pilots=(None, 100)):
    """every route under the pilot's own verdict and with the bounded order forced (100): the oracle's bytes, hence each other's"""
    for pilot in pilots:
        for route, env in ROUTES.items():
            got = _encode(itw, gpu, img, env, pilot)
            assert first_mismatch(got, want, 16) is None, (route, pilot, first_mismatch(got, want, 16))


def _tiled(oracle, base, ry, rx):
    """`base` (sides multiples of 4) repeated ry x rx times and the oracle's blocks of it: the oracle encodes the base once"""
    h, w = base.shape[0] // 4 * 4, base.shape[1] // 4 * 4
    base = np.ascontiguousarray(base[:h, :w])
    want = oracle.encode_mt("bc7", base, "slow").reshape(h // 4, w // 4, 16)
    return np.ascontiguousarray(np.tile(base, (ry, rx, 1))), np.ascontiguousarray(np.tile(want, (ry, rx, 1))).reshape(-1)


def test_crop_of_the_bench_surface(itw, gpu, oracle):
    from itw_amd import surfaces
    img = np.ascontiguousarray(surfaces.ldr_smooth(4096, 4096, surfaces.SEED)[1024:2048, 2048:3072])
    assert img.shape[0] * img.shape[1] // 16 >= 65536
    _check(itw, gpu, img, oracle.encode_mt("bc7", img, "slow"))


@pytest.mark.parametrize("name", ["baboon", "monkey"])
def test_photographs_tiled_to_the_fused_shape(itw, gpu, oracle, golden_inputs, name):
    base = golden_inputs[name]
    by, bx = base.shape[0] // 4, base.shape[1] // 4
    ry = rx = 1
    while by * ry * bx * rx < 65536:
        if by * ry <= bx * rx:
            ry *= 2
        else:
            rx *= 2
    img, want = _tiled(oracle, base, ry, rx)
    assert img.shape[0] * img.shape[1] // 16 >= 65536
    _check(itw, gpu, img, want)


def test_adversarial_blocks_two_bands(itw, gpu, oracle, deep):
    """flat, two-level and collinear blocks: bounds of exactly 0 and massive error ties between shapes -- the atomic merge has to keep the
    reference's rank-key order.  33 rows of 321 blocks: two bands, a listed count that is no multiple of 64."""
    img, want = _tiled(oracle, adversarial_blocks(np.random.default_rng(20260927)), 33, 1)
    assert img.shape[0] * img.shape[1] // 16 >= 32 * 256
    _check(itw, gpu, img, want)


def test_adversarial_blocks_one_band(itw, gpu, oracle, deep):
    img = adversarial_blocks(np.random.default_rng(5))
    assert img.shape[0] * img.shape[1] // 16 < 32 * 256
    _check(itw, gpu, img, oracle.encode_mt("bc7", img, "slow"))


@pytest.mark.parametrize("h,w", [(92, 100), (516, 604)], ids=["one_band_575_blocks", "two_bands_partial_chunk"])
def test_mixed_content_at_odd_sizes(itw, gpu, oracle, deep, golden_inputs, h, w):
    """noise over smooth fields, a photograph, few-level content and two-colour blocks; block counts that are multiples of neither 64 nor
    256 (23 x 25 and 129 x 151 blocks), so the lists, the buckets' last tiles and the second list end inside a wave"""
    from test_gpu_bc7_bound import _mixed_content
    img = _mixed_content(golden_inputs, h, w)
    assert (img.shape[0] // 4) * (img.shape[1] // 4) % 64 != 0
    _check(itw, gpu, img, oracle.encode_mt("bc7", img, "slow"))


def test_custom_structs_on_the_pair_route(itw, gpu, oracle, deep, golden_inputs):
    """only one of modes 1 / 3 scanned, no refinement, mode 2 off: the pair scan's single-mode branches and a commit without iterations"""
    from test_gpu_bc7_bound import _mixed_content
    img = _mixed_content(golden_inputs, 260, 516)
    for variant in range(4):
        s, o = itw.bc7_profile("slow"), oracle.bc7_profile("slow")
        for t in (s, o):
            if variant == 0:
                t.fastSkipTreshold_mode1 = 0
            if variant == 1:
                t.fastSkipTreshold_mode3 = 0
            if variant == 2:
                for i in range(8):
                    t.refineIterations[i] = 0
            if variant == 3:
                t.skip_mode2 = 1
                t.mode_selection[2] = 0
        want = oracle.encode_mt("bc7", img, o)
        import torch
        for route, env in ROUTES.items():
            saved = {k: os.environ.pop(k, None) for k in ("ITW_BC7_PAIRS", "ITW_BC7_PAIR_CAP")}
            os.environ.update(env)
            itw.set_bc7_pilot(100)
            try:
                out = itw.compress("bc7", torch.from_numpy(img).to(gpu), s)
                torch.cuda.synchronize()
            finally:
                itw.set_bc7_pilot(None)
                for k in saved:
                    os.environ.pop(k, None)
                    if saved[k] is not None:
                        os.environ[k] = saved[k]
            assert first_mismatch(out.cpu().numpy(), want, 16) is None, (variant, route, first_mismatch(out.cpu().numpy(), want, 16))
