"""examples/encode_dds.cpp --signed-normal: a raw file of int8, half or float texels to a BC4_SNORM / BC5_SNORM DDS whose payload is the
Python calls' (itwCompressNormalMapBC5S, itwCompressSignedNormalMapChain, itwCompressSignedNormalMapMipped); and --normal with bc5_snorm
keeps writing the bytes it wrote before the signed path existed (the plugin's biased 8-bit convention)."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import _normal_snorm as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "encode_dds")
pytestmark = pytest.mark.gpu
FLAG = {"int8": "int8", "half": "half", "float": "float"}
# SHA-256 of the file `encode_dds --normal flipy,normalize bc5_snorm 30 37` wrote on the parent commit for _biased_input()
PARENT_NORMAL_BC5_SNORM_SHA256 = "e26ebcdafe3ad77aa0cb769a18f54174bf2ef2a4a859c34b28a6f41be1ac3e69"


def _biased_input():
    return np.random.default_rng(12).integers(0, 256, (37, 30, 4), dtype=np.uint8)


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


def _host(kind, h, w, seed):
    a = S.content(kind, h, w, seed)
    return a.view(np.int16) if a.dtype == np.uint16 else a


@pytest.mark.parametrize("kind", S.KINDS)
def test_bc5_snorm_payload_is_the_fused_calls(itw, gpu, tmp_path, kind):
    img = _host(kind, 37, 30, 1)
    f = _run(tmp_path, img, "bc5_snorm", "--signed-normal", FLAG[kind] + ",flipy,normalize")
    d, off = _header(itw, f)
    assert d.dxgi_format == 84 and (d.width, d.height, d.mip_levels, d.is_cubemap) == (30, 37, 1, 0)
    assert np.array_equal(f[off:], itw.compress_normal_map_snorm(img, flip_y=True, normalize=True))


@pytest.mark.parametrize("kind", S.KINDS)
def test_bc4_snorm_goes_through_the_chain_call_with_one_image(itw, gpu, tmp_path, kind):
    img = _host(kind, 21, 18, 2)
    f = _run(tmp_path, img, "bc4_snorm", "--signed-normal", FLAG[kind] + ",flipx")
    d, off = _header(itw, f)
    assert d.dxgi_format == 81 and (d.width, d.height) == (18, 21)
    ok, want = itw.compress_chain_normal_snorm("bc4_snorm", [img], flip_x=True)
    assert ok and np.array_equal(f[off:], want)


@pytest.mark.parametrize("kind", S.KINDS)
def test_mips_and_cube_cross(itw, gpu, tmp_path, kind):
    img = _host(kind, 24, 32, 3)                       # a horizontal cross of 8 x 8 faces
    faces = [np.ascontiguousarray(v) for v in itw.cube_cross_faces(img)]
    f = _run(tmp_path, img, "bc5_snorm", "--signed-normal", FLAG[kind] + ",normalize", "--cube-cross", "--mips")
    d, off = _header(itw, f)
    assert d.dxgi_format == 84 and (d.width, d.height, d.mip_levels, d.is_cubemap) == (8, 8, 4, 1)
    ok, want = itw.compress_mipped_normal_snorm("bc5_snorm", faces, normalize=True)
    assert ok and np.array_equal(f[off:], want)
    f = _run(tmp_path, img, "bc5_snorm", "--signed-normal", FLAG[kind], "--cube-cross")
    d, off = _header(itw, f)
    assert (d.width, d.height, d.mip_levels, d.is_cubemap) == (8, 8, 1, 1)
    ok, want = itw.compress_chain_normal_snorm("bc5_snorm", faces)
    assert ok and np.array_equal(f[off:], want)
    f = _run(tmp_path, img, "bc4_snorm", "--signed-normal", FLAG[kind] + ",flipx,flipy,normalize", "--mips", "3")
    d, off = _header(itw, f)
    assert d.dxgi_format == 81 and (d.width, d.height, d.mip_levels, d.is_cubemap) == (32, 24, 3, 0)
    ok, want = itw.compress_mipped_normal_snorm("bc4_snorm", img, levels=3, ops=7)
    assert ok and np.array_equal(f[off:], want)


def test_signed_normal_is_refused_where_it_does_not_belong(tmp_path):
    raw = tmp_path / "in.raw"
    np.zeros((8, 8, 4), np.float32).tofile(raw)
    for flags, fmt in ((["--signed-normal", "float"], "bc5"), (["--signed-normal", "float", "--normal", "flipx"], "bc5_snorm"),
                       (["--signed-normal", "double"], "bc5_snorm"), (["--signed-normal", "flipx"], "bc5_snorm")):
        r = subprocess.run([EXE, *flags, fmt, "8", "8", str(raw), str(tmp_path / "out.dds")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and not (tmp_path / "out.dds").exists(), (flags, fmt, r.stderr)


def test_normal_with_bc5_snorm_writes_what_it_wrote_before(tmp_path):
    f = _run(tmp_path, _biased_input(), "bc5_snorm", "--normal", "flipy,normalize")
    assert hashlib.sha256(f.tobytes()).hexdigest() == PARENT_NORMAL_BC5_SNORM_SHA256
