"""The staged runs of a host-pointer call (csrc/abi.hip compress_runs(), cut by csrc/host_runs.hpp) at the smallest sizes they exist at:
64 x 256 texels is 64 block rows, the least ITW_HOST_RUNS cuts.  The knob is read per call, so it is set in-process around the calls.  For
BC7 the runs are bands -- each run's kernels on one of two streams, in its own slice of the workspace, the first one leaving the pilot's
verdict -- and every byte of every call is compared with the oracle: after one another on changing content (slices, events and verdict
reused), from a pitched and a bottom-up source, into a device destination, as one-row runs; BC6H `fast` runs without bands, and BC1 (one
run by default) cut by ITW_HOST_CHUNKS.  These tests compare bytes only; which launch shape each run took -- bands, wide runs, the probe --
is pinned at this size by tests/test_gpu_launch_switches.py, which reads the route witness of the hooks build, and at 2048 x 4096 by the
alternation of tests/test_gpu_host_pointer_runs.py."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from conftest import first_mismatch

pytestmark = pytest.mark.gpu
H, W = 256, 64
RUNS = "0.125,0.625"                                      # block rows [0, 8) [8, 40) [40, 64)


@contextlib.contextmanager
def knob(name, value):
    os.environ[name] = value
    try:
        yield
    finally:
        del os.environ[name]


@pytest.fixture(scope="module")
def cases(oracle, golden_inputs):
    """name -> (format, profile, texels, the oracle's stream); computed once, read-only"""
    from itw_amd import surfaces
    smooth = surfaces.ldr_smooth(H, W)
    photo = np.ascontiguousarray(np.tile(golden_inputs["baboon"][:128, :W], (H // 128, 1, 1)))
    hdr = surfaces.hdr_smooth(H, W)
    out = {}
    for prof in ("slow", "alpha_slow"):
        out["smooth", prof] = ("bc7", prof, smooth, oracle.encode("bc7", smooth, prof).reshape(-1))
        out["photo", prof] = ("bc7", prof, photo, oracle.encode("bc7", photo, prof).reshape(-1))
        flipped = np.ascontiguousarray(smooth[::-1])
        out["flipped", prof] = ("bc7", prof, flipped, oracle.encode("bc7", flipped, prof).reshape(-1))
    out["bc6h"] = ("bc6h", "fast", hdr, oracle.encode("bc6h", hdr, "fast").reshape(-1))
    out["bc1"] = ("bc1", None, smooth, oracle.encode("bc1", smooth, None).reshape(-1))
    for v in out.values():
        v[2].setflags(write=False); v[3].setflags(write=False)
    return out


def check(itw, case, img=None, what=""):
    fmt, prof, texels, want = case
    got = itw.compress_numpy(fmt, texels if img is None else img, prof)
    assert got.size == want.size and first_mismatch(got, want, itw.BYTES_PER_BLOCK[fmt]) is None, (fmt, prof, what, first_mismatch(got, want, itw.BYTES_PER_BLOCK[fmt]))


@pytest.mark.parametrize("prof", ["slow", "alpha_slow"])
def test_three_bands_on_changing_content(itw, gpu, cases, prof):
    with knob("ITW_HOST_RUNS", RUNS):
        for k, name in enumerate(("smooth", "photo", "smooth")):
            check(itw, cases[name, prof], what=(k, name))


@pytest.mark.parametrize("prof", ["slow", "alpha_slow"])
def test_three_bands_from_a_pitched_source(itw, gpu, cases, prof):
    texels = cases["smooth", prof][2]
    wide = np.zeros((H, W + 5, 4), np.uint8)              # rows 20 bytes further apart than their texels
    wide[:, :W] = texels
    assert wide.strides[0] == W * 4 + 20
    with knob("ITW_HOST_RUNS", RUNS):
        check(itw, cases["smooth", prof], wide[:, :W], "pitched")


@pytest.mark.parametrize("prof", ["slow", "alpha_slow"])
def test_three_bands_from_a_bottom_up_source(itw, gpu, cases, prof):
    _, _, flipped, want = cases["flipped", prof]
    img = np.ascontiguousarray(flipped[::-1])             # read from its last row upwards this is `flipped`
    surf = itw.RgbaSurface(img.ctypes.data + (H - 1) * img.strides[0], W, H, -img.strides[0])
    out = np.zeros(want.size, np.uint8)
    st = itw.bc7_profile(prof)
    with knob("ITW_HOST_RUNS", RUNS):
        itw.lib().CompressBlocksBC7(C.byref(surf), out.ctypes.data, C.byref(st))
    assert first_mismatch(out, want, 16) is None, (prof, first_mismatch(out, want, 16))


@pytest.mark.parametrize("prof", ["slow", "alpha_slow"])
def test_three_bands_into_a_device_destination(itw, gpu, cases, prof):
    import torch
    _, _, img, want = cases["smooth", prof]
    surf = itw.RgbaSurface(img.ctypes.data, W, H, img.strides[0])
    d_out = torch.zeros(want.size, dtype=torch.uint8, device=gpu)
    st = itw.bc7_profile(prof)
    with knob("ITW_HOST_RUNS", RUNS):
        itw.lib().CompressBlocksBC7(C.byref(surf), C.c_void_p(d_out.data_ptr()), C.byref(st))
    torch.cuda.synchronize()
    assert first_mismatch(d_out.cpu().numpy(), want, 16) is None, (prof, first_mismatch(d_out.cpu().numpy(), want, 16))


@pytest.mark.parametrize("prof", ["slow", "alpha_slow"])
def test_one_row_runs(itw, gpu, cases, prof):
    with knob("ITW_HOST_RUNS", "0,0,0"):                  # block rows [0, 1) [1, 2) [2, 3) [3, 64)
        check(itw, cases["smooth", prof], what="one-row runs")
        check(itw, cases["photo", prof], what="one-row runs")


def test_runs_without_bands_bc6h(itw, gpu, cases):
    with knob("ITW_HOST_RUNS", RUNS):
        for k in range(2):
            check(itw, cases["bc6h"], what=k)


def test_runs_of_a_pcie_bound_format_bc1(itw, gpu, cases):
    with knob("ITW_HOST_CHUNKS", "4"):
        for k in range(2):
            check(itw, cases["bc1"], what=k)
