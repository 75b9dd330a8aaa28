"""examples/encode_dds.cpp, the normal-map and cube-cross stages of the save path above the C ABI: `--normal` writes the fused call's
payload for bc5 and the chain call's for another format; `--cube-cross` writes a six-face DDS that itwDdsReadHeader reads as a cube."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _normal_prep as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "encode_dds")
pytestmark = pytest.mark.gpu


def _run(tmp_path, img, fmt, *flags):
    raw, dds = tmp_path / "in.raw", tmp_path / "out.dds"
    np.ascontiguousarray(img).tofile(raw)
    h, w = img.shape[:2]
    r = subprocess.run([EXE, *flags, fmt, str(w), str(h), str(raw), str(dds)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return np.fromfile(dds, dtype=np.uint8)


def _header(itw, f):
    d = itw.DdsDesc()
    off = itw.lib().itwDdsReadHeader(f.ctypes.data, f.size, C.byref(d))
    assert off in (128, 148)
    return d, off


def test_normal_bc5_payload_is_the_fused_calls(itw, gpu, tmp_path):
    import torch
    img = np.random.default_rng(3).integers(0, 256, (37, 30, 4), dtype=np.uint8)
    f = _run(tmp_path, img, "bc5", "--normal", "flipy,normalize")
    d, off = _header(itw, f)
    assert d.dxgi_format == 83 and (d.width, d.height, d.mip_levels, d.is_cubemap) == (30, 37, 1, 0)
    want = itw.compress_normal_map(torch.from_numpy(img).to(gpu), flip_y=True, normalize=True).cpu().numpy()
    assert np.array_equal(f[off:], want)
    assert np.array_equal(want, itw.compress("bc5", torch.from_numpy(N.prepare_rgba8(img, 6)).to(gpu)).cpu().numpy())


def test_normal_other_format_goes_through_the_chain_call(itw, gpu, tmp_path):
    img = np.random.default_rng(4).integers(0, 256, (21, 18, 4), dtype=np.uint8)
    f = _run(tmp_path, img, "bc7_veryfast", "--normal", "flipx")
    d, off = _header(itw, f)
    assert d.dxgi_format == 98 and (d.width, d.height) == (20, 24)
    ok, want = itw.compress_chain("bc7", [N.prepare_rgba8(img, 1)], "veryfast")
    assert ok and np.array_equal(f[off:], want)


@pytest.mark.parametrize("h,w", [(24, 32), (32, 24)])
def test_cube_cross_writes_a_six_face_dds(itw, gpu, tmp_path, h, w):
    img = np.random.default_rng(h).integers(0, 256, (h, w, 4), dtype=np.uint8)
    f = _run(tmp_path, img, "bc5", "--cube-cross", "--normal", "normalize")
    d, off = _header(itw, f)
    assert d.dxgi_format == 83 and (d.width, d.height, d.mip_levels, d.is_cubemap, d.array_size) == (8, 8, 1, 1, 1)
    faces = [np.ascontiguousarray(N.prepare_rgba8(v, 4)) for v in itw.cube_cross_faces(img)]
    ok, want = itw.compress_chain("bc5", faces)
    assert ok and f.size == off + want.size and np.array_equal(f[off:], want)
