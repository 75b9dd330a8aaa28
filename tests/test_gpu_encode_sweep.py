"""The encoders over the sources of tests/_encode_sweep.py, on which every BC7 (mode, partition / rotation + index selector) combination and
every BC6H (mode, partition) pair wins blocks (tests/test_encode_sweep.py counts that on the oracle's streams): every preset and a set of
settings structs through both launch shapes (csrc/bc7.hip, csrc/bc6h.hip: the fused "deep" kernels, the split-scan "wide" ones, the ranked
lists in registers and in LDS, the per-family kernels), `slow` and `alpha_slow` through the bounded orders with their block lists and through
bc7_rot_tasks and its alternatives, in one band and in two; BC1 / BC3 / BC4 / BC5 over texels that all lie on interpolation levels.  The sources
are decoded blocks, so they are full of exact ties between modes and between partitions: the reference's order with strict `<` decides
thousands of blocks on every route.  Every comparison is the oracle's bytes, and each test first holds the oracle's stream to the pinned number
of combinations, so it cannot run on content that lost its coverage."""
import numpy as np
import pytest

import _encode_sweep as es
from conftest import first_mismatch
from test_encode_sweep import BC6H_PRESETS, BC7_PRESETS, COMBINATION, oracle_stream, pins, settings_of
from test_gpu_bc7_rot_tasks import ROUTES, _encode as encode_on_route

pytestmark = pytest.mark.gpu

SHAPES = ["deep", "wide"]


@pytest.fixture
def paths(itw):
    yield itw.set_bc7_path
    itw.set_bc7_path("auto")


@pytest.fixture(scope="module")
def on_device(gpu):
    """the two sources as device tensors, uploaded once"""
    import torch
    return {"bc7": torch.from_numpy(es.bc7_source().copy()).to(gpu), "bc6h": torch.from_numpy(es.bc6h_source().view(np.int16).copy()).to(gpu)}


@pytest.fixture(scope="module")
def wanted(oracle):
    """wanted(fmt, name): the oracle's stream of the format's source under a preset or a variant of _encode_sweep, encoded once, and held to
    the pinned number of combinations"""
    pinned = pins()["combinations"]

    def get(fmt, name):
        blocks = oracle_stream(oracle, fmt, name)
        assert len(set(COMBINATION[fmt](blocks))) == pinned[fmt][name], (fmt, name)
        return blocks
    return get


def _encode(itw, fmt, src, settings):
    import torch
    out = itw.compress(fmt, src, settings)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _where(fmt, got, want, what):
    """the (mode, field) the oracle chose and the device wrote for the first differing block, with first_mismatch's index and bytes"""
    g, w = np.asarray(got).reshape(-1, 16), np.asarray(want).reshape(-1, 16)
    i = int(np.nonzero((g != w).any(axis=1))[0][0])
    return what, "wanted (mode, field)", COMBINATION[fmt](w[i]), "got", COMBINATION[fmt](g[i]), first_mismatch(got, want, 16)


# ---- BC7 -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("prof", BC7_PRESETS)
def test_bc7_presets(itw, gpu, paths, on_device, wanted, prof, shape):
    want = wanted("bc7", prof)
    paths(shape)
    got = _encode(itw, "bc7", on_device["bc7"], prof)
    assert first_mismatch(got, want, 16) is None, _where("bc7", got, want, (prof, shape))


def _geometry(src, want, name):
    """one_band: the source as it is, 72 x 64 blocks; one_band_partial_wave: without its last block column, 72 x 63 = 4 536 blocks, no
    multiple of 64, so every list and the surface itself end inside a wave; two_bands: twice on top of itself, 9 216 blocks"""
    rows = want.reshape(-1, 64, 16)
    if name == "one_band_partial_wave":
        return src[:, :252].contiguous(), np.ascontiguousarray(rows[:, :63]).reshape(-1)
    if name == "two_bands":
        return src.repeat(2, 1, 1), np.concatenate([want, want])
    return src, want


@pytest.mark.parametrize("geometry", ["one_band", "one_band_partial_wave", "two_bands"])
@pytest.mark.parametrize("prof", ["slow", "alpha_slow"])
def test_bc7_slow_orders_on_every_route(itw, gpu, paths, on_device, wanted, prof, geometry):
    """the pilot's own verdict and the bounded order forced, each over the four per-call routes of modes 4/5 and of the pair lists"""
    whole = wanted("bc7", prof)
    src, want = _geometry(on_device["bc7"], whole, geometry)
    blocks = src.shape[0] * src.shape[1] // 16
    assert (blocks >= 32 * 256) == (geometry == "two_bands") and (blocks % 64 != 0) == (geometry == "one_band_partial_wave")
    assert set(es.bc7_combination(want)) == set(es.bc7_combination(whole))            # the cut column takes no combination along
    paths("deep")
    for pilot in (None, 100):
        for route, env in ROUTES.items():
            got = encode_on_route(itw, gpu, src, env, pilot, prof)
            assert first_mismatch(got, want, 16) is None, _where("bc7", got, want, (prof, geometry, route, pilot))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("variant", list(es.BC7_VARIANTS))
def test_bc7_settings_structs(itw, gpu, paths, on_device, wanted, variant, shape):
    """`alpha_slow` (four channels, all eight modes open) with ranked lists of 16 (ranked in registers), 17 (LDS keys, per-family kernels;
    the wide shape hands these to the deep one), 1 and 64 shapes, each mode family alone, each first rotation of modes 4/5.  With a short
    list the partition that wins is the one the rank key puts first: another stream than the whole table's, decided per partition."""
    want = wanted("bc7", variant)
    paths(shape)
    got = _encode(itw, "bc7", on_device["bc7"], settings_of(itw, "bc7", variant))
    assert first_mismatch(got, want, 16) is None, _where("bc7", got, want, (variant, shape))


# ---- BC6H ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", BC6H_PRESETS + list(es.BC6H_VARIANTS))
def test_bc6h_presets_and_list_lengths(itw, gpu, paths, on_device, wanted, name, shape):
    """the five presets, and `slow` with ranked lists of 1, 2, 31 and 32 partitions, with and without the two-region refinement"""
    want = wanted("bc6h", name)
    paths(shape)
    got = _encode(itw, "bc6h", on_device["bc6h"], settings_of(itw, "bc6h", name))
    assert first_mismatch(got, want, 16) is None, _where("bc6h", got, want, (name, shape))


# ---- BC1, BC3, BC4, BC5 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["bc1", "bc3", "bc4", "bc5"])
def test_small_formats_on_interpolation_levels(itw, gpu, oracle, fmt):
    """every texel on a level of the 65 536 BC4 / BC5 endpoint pairs and of the 565 corner colours in both orders: index rounding and the
    endpoint-order conventions decide every block"""
    import torch
    img = es.small_sources()[fmt]
    want = oracle.encode_mt(fmt, img)
    got = _encode(itw, fmt, torch.from_numpy(img.copy()).to(gpu), None)
    assert got.size == want.size
    assert first_mismatch(got, want, 8) is None, (fmt, first_mismatch(got, want, 8))
