"""search_02 (csrc/bc7.hip), the modes 0/2 head scan: it visits the three-subset shapes in the order of csrc/bc7_f02_schedule.h and takes a
subset's error from one of two caches wherever an earlier shape had the same texel mask -- mode 2's in four registers, mode 0's in four words
of the lane's LDS column -- skipping the subset outright where it needs nothing else.

The hook (itwTestBc7F02Scan) runs the scan of every block in that order with both caches and again in table order with nothing cached, and
leaves every per-shape error of both modes: a stale or mixed-up slot shows there even where the wrong value does not happen to win.
Through the ordinary entry point, fused launch shape, the stream must be the oracle's byte for byte at
    12 x 8      one workgroup, 250 idle lanes
    128 x 96    three workgroups, the single-band route
    604 x 516   two bands, a ragged last workgroup
on the bench surface's generator, on noise, and on a surface on which every three-subset shape wins mode 2 and each of the first 16 wins
mode 0 (tests/_f02_surfaces.py; the condition is asserted on the oracle's stream wherever the surface has room for the 80 combinations),
under `slow` and `alpha_slow`, each call made twice."""
import numpy as np
import pytest

import _f02_surfaces as fs
from conftest import first_mismatch

pytestmark = pytest.mark.gpu

SIZES = ((8, 12), (96, 128), (516, 604))                             # rows x columns
CONTENTS = ("smooth", "noise", "partitions")


def _surface(name, h, w):
    from itw_amd import surfaces
    return {"smooth": surfaces.ldr_smooth, "noise": fs.noise, "partitions": fs.partitions}[name](h, w)


def test_cached_and_uncached_scans_give_every_shape_the_same_error(itw, gpu):
    """512 blocks (128 x 64 pixels), the left half noise (all errors distinct), the right half the bench generator's"""
    import torch
    from itw_amd import surfaces
    img = surfaces.ldr_smooth(64, 128).copy()
    img[:, :64] = fs.noise(64, 64)
    got = itw.bc7_f02_scan(torch.from_numpy(img).to(gpu)).cpu().numpy()
    assert got.shape == (512, 2, 84)
    cached, plain = got[:, 0], got[:, 1]
    assert (plain[:, 4:] >= 0).all() and (cached[:, 4:] >= 0).all()              # every error was written
    bad = np.argwhere(cached[:, 4:] != plain[:, 4:])
    assert bad.size == 0, ("block, k (k < 16: mode 0 shape k; else mode 2 shape k - 16)", bad[:8].tolist(),
                           cached[bad[0][0], 4 + bad[0][1]], plain[bad[0][0], 4 + bad[0][1]])
    assert np.array_equal(cached[:, :4], plain[:, :4])
    # the winners are what the per-shape errors say: lowest error, then lowest table index
    for mode_errs, col in ((plain[:, 4:20], 0), (plain[:, 20:84], 2)):
        assert np.array_equal(plain[:, col], mode_errs.min(axis=1))
        assert np.array_equal(plain[:, col + 1], 64 + mode_errs.argmin(axis=1))
    # the noise half is there for distinct errors: a slot read in place of another cannot go unnoticed
    distinct = np.mean([len(set(r[20:84].tolist())) for r in plain.reshape(16, 32, 84)[:, :16].reshape(-1, 84)])
    assert distinct > 60, distinct


@pytest.fixture(scope="module")
def deep(itw):
    """the fused launch shape whatever the size"""
    itw.set_bc7_path("deep")
    yield
    itw.set_bc7_path("auto")


@pytest.mark.parametrize("prof", fs.PROFILES)
@pytest.mark.parametrize("name", CONTENTS)
@pytest.mark.parametrize("h,w", SIZES, ids=[f"{w}x{h}" for h, w in SIZES])
def test_same_bytes_as_the_oracle(itw, gpu, oracle, deep, h, w, name, prof):
    import torch
    img = _surface(name, h, w)
    want = oracle.encode_mt("bc7", img, prof)
    if name == "partitions" and (h // 4) * (w // 4) >= len(fs.COMBINATIONS):
        missing = fs.missing_winners(want)                           # a condition on the input: otherwise the case proves nothing
        assert not missing, sorted(missing)
    src = torch.from_numpy(img).to(gpu)
    for call in ("first", "again"):
        got = itw.compress("bc7", src, prof)
        torch.cuda.synchronize()
        m = first_mismatch(got.cpu().numpy(), want, 16)
        assert m is None, (call, m)
