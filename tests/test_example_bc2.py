"""examples/encode_dds.cpp with the format bc2: the file's payload is the binding's, its header is a DXT3 file's (DX10 with 74 for a cube's
array does not arise here), --decode reads it back, and the flags are refused where they have no meaning."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _dxtex_bc2 as B2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "encode_dds")


def _run(tmp_path, img, fmt, *flags):
    raw, out = tmp_path / "in.raw", tmp_path / "out.dds"
    np.ascontiguousarray(img).tofile(raw)
    h, w = img.shape[:2]
    return subprocess.run([EXE, *flags, fmt, str(w), str(h), str(raw), str(out)], capture_output=True, text=True, timeout=300), out


def _payload(itw, out):
    f = np.fromfile(out, dtype=np.uint8)
    d = itw.DdsDesc()
    off = itw.lib().itwDdsReadHeader(f.ctypes.data, f.size, C.byref(d))
    assert off == 128 and f[84:88].tobytes() == b"DXT3" and d.dxgi_format == itw.DXGI_FORMAT["bc2"]      # the legacy header of a BC2 file
    return d, f[off:]


@pytest.mark.parametrize("fmt,flags,word", [
    ("bc2", ("--bc-dither", "b"), "--bc-dither takes"),
    ("bc2", ("--normal", "normalize"), "not with --normal"),
    ("bc2", ("--refine", "slow", "100"), "not with --normal or --refine"),
    ("bc2:0.5", (), "unknown format"),
    ("bc3", ("--bc-dither", "a"), "bc1a's flags (and bc2's)"),
])
def test_flags_are_refused_where_they_mean_nothing(tmp_path, fmt, flags, word):
    r, out = _run(tmp_path, np.zeros((8, 8, 4), np.uint8), fmt, *flags)
    assert r.returncode == 2 and word in r.stderr and not out.exists(), (r.returncode, r.stderr)


def test_decode_refuses_a_truncated_dxt3_file(itw, tmp_path):
    """--decode reads a DXT3 header (before this format the file was "not a BCn DDS file this library reads") and checks the payload's
    length before any device work."""
    f = itw.dds_file("bc2", 8, 8, [np.zeros(64, np.uint8)])
    assert f[84:88].tobytes() == b"DXT3"
    path = tmp_path / "short.dds"
    f[:-16].tofile(path)
    r = subprocess.run([EXE, "--decode", str(path), str(tmp_path / "out.raw")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "truncated" in r.stderr and not (tmp_path / "out.raw").exists(), r.stderr


@pytest.mark.gpu
def test_single_image_with_flags_measured_and_decoded_back(itw, gpu, tmp_path):
    img = B2.cutout(30, 41, 5)
    r, out = _run(tmp_path, img, "bc2", "--bc-dither", "rgb,a", "--bc-uniform", "--measure")
    assert r.returncode == 0, r.stderr
    d, got = _payload(itw, out)
    assert (d.width, d.height, d.mip_levels) == (41, 30, 1)                              # a DirectXTex format: the image's own size
    ok, want = itw.compress_image("bc2", img, settings=itw.Bc1aSettings(0.5, True, True, True))
    assert ok and np.array_equal(got, want)
    assert r.stdout.startswith("image 0: 41x30 bc2 psnr ")
    back = tmp_path / "back.raw"
    r = subprocess.run([EXE, "--decode", str(out), str(back)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    texels = np.fromfile(back, dtype=np.uint8).reshape(30, 41, 4)
    assert np.array_equal(texels, B2.np_decode(want, 30, 41))
    assert r.stdout.startswith("image 0: 41 30 min_alpha %d" % int(texels[..., 3].min()))


@pytest.mark.gpu
def test_mipped_cutout_writes_the_payload_of_the_python_path(itw, gpu, tmp_path):
    img = B2.cutout(24, 40, 21)
    r, out = _run(tmp_path, img, "bc2", "--mips", "--alpha-coverage", "128", "--bc-dither", "a")
    assert r.returncode == 0, r.stderr
    d, got = _payload(itw, out)
    assert (d.width, d.height, d.mip_levels) == (40, 24, 6)
    ok, want = itw.compress_mipped("bc2", img, alpha_coverage=128, settings=itw.Bc1aSettings(dither_a=True))
    assert ok and np.array_equal(got, want)
    back = tmp_path / "back.raw"
    r = subprocess.run([EXE, "--decode", str(out), str(back)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and len(r.stdout.splitlines()) == 6, r.stdout + r.stderr
