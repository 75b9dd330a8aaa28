"""examples/encode_dds.cpp --mips: the base image (or the six faces of a cube cross) through itwCompressImageMipped into a mipped DDS --
a KTX file for ETC1 -- whose header reads back with the right mip count and whose payload is the binding's compress_mipped."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "encode_dds")
pytestmark = pytest.mark.gpu


def _run(tmp_path, img, fmt, *flags):
    raw, out = tmp_path / "in.raw", tmp_path / "out.bin"
    np.ascontiguousarray(img).tofile(raw)
    h, w = img.shape[:2]
    r = subprocess.run([EXE, *flags, fmt, str(w), str(h), str(raw), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return np.fromfile(out, dtype=np.uint8)


def _header(itw, f):
    d = itw.DdsDesc()
    off = itw.lib().itwDdsReadHeader(f.ctypes.data, f.size, C.byref(d))
    assert off in (128, 148)
    return d, off


def test_mips_writes_a_full_chain(itw, gpu, tmp_path):
    img = np.random.default_rng(1).integers(0, 256, (12, 20, 4), dtype=np.uint8)
    f = _run(tmp_path, img, "bc7_ultrafast", "--mips")
    d, off = _header(itw, f)
    assert d.dxgi_format == 98 and (d.width, d.height, d.mip_levels, d.is_cubemap) == (20, 12, 5, 0)
    ok, want = itw.compress_mipped("bc7", img, profile="ultrafast")
    assert ok and f.size == off + want.size == itw.lib().itwDdsFileBytes(C.byref(d)) and np.array_equal(f[off:], want)


def test_mips_with_a_level_count_a_normal_map_and_a_cube_cross(itw, gpu, tmp_path):
    img = np.random.default_rng(2).integers(0, 256, (48, 64, 4), dtype=np.uint8)           # faces of 16 x 16
    f = _run(tmp_path, img, "bc5", "--cube-cross", "--mips", "3", "--normal", "flipx,flipy,normalize")
    d, off = _header(itw, f)
    assert d.dxgi_format == 83 and (d.width, d.height, d.mip_levels, d.is_cubemap, d.array_size) == (16, 16, 3, 1, 1)
    faces = [np.ascontiguousarray(v) for v in itw.cube_cross_faces(img)]
    ok, want = itw.compress_mipped("bc5", faces, levels=3, normal_ops=7)
    assert ok and f.size == off + want.size and np.array_equal(f[off:], want)


def test_mips_half_floats(itw, gpu, tmp_path):
    img = np.random.default_rng(3).normal(0.5, 0.25, (32, 32, 4)).astype(np.float16).view(np.uint16)
    f = _run(tmp_path, img, "bc6h_veryfast", "--mips")
    d, off = _header(itw, f)
    assert d.dxgi_format == 95 and (d.width, d.height, d.mip_levels) == (32, 32, 6)
    ok, want = itw.compress_mipped("bc6h", img, profile="veryfast")
    assert ok and np.array_equal(f[off:], want)


def test_mips_etc1_writes_a_ktx(itw, gpu, tmp_path):
    img = np.random.default_rng(4).integers(0, 256, (16, 8, 4), dtype=np.uint8)
    f = _run(tmp_path, img, "etc1_slow", "--mips")
    k = itw.KtxDesc()
    assert itw.lib().itwKtxReadHeader(f.ctypes.data, f.size, C.byref(k)) == 64
    assert (k.width, k.height, k.mip_levels, k.is_cubemap) == (8, 16, 5, 0)
    ok, want = itw.compress_mipped("etc1", img)
    assert ok
    got = []
    for i in range(5):
        off = C.c_size_t()
        n = itw.lib().itwKtxImage(C.byref(k), i, None, None, C.byref(off))
        got.append(f[off.value:off.value + n])
    assert np.array_equal(np.concatenate(got), want)


def test_mips_refuses_too_many_levels(tmp_path):
    raw = tmp_path / "in.raw"
    np.zeros((8, 8, 4), np.uint8).tofile(raw)
    r = subprocess.run([EXE, "--mips", "5", "bc1", "8", "8", str(raw), str(tmp_path / "out.dds")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "levels" in r.stderr and not (tmp_path / "out.dds").exists()
