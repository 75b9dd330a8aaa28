"""examples/encode_dds.cpp with the format bc1a[:<alpha_ref>]: the file's payload is the binding's, its header says BC1 (DXGI 71), and the
flags are refused where they have no meaning."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _alpha_mips as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "encode_dds")


def _run(tmp_path, img, fmt, *flags):
    raw, out = tmp_path / "in.raw", tmp_path / "out.bin"
    np.ascontiguousarray(img).tofile(raw)
    h, w = img.shape[:2]
    return subprocess.run([EXE, *flags, fmt, str(w), str(h), str(raw), str(out)], capture_output=True, text=True, timeout=300), out


def _payload(itw, out):
    f = np.fromfile(out, dtype=np.uint8)
    d = itw.DdsDesc()
    off = itw.lib().itwDdsReadHeader(f.ctypes.data, f.size, C.byref(d))
    assert off == 128 and f[84:88].tobytes() == b"DXT1" and d.dxgi_format == 71          # the legacy header of a BC1 file
    return d, f[off:]


@pytest.mark.gpu
def test_mipped_cutout_writes_the_payload_of_the_python_path(itw, gpu, tmp_path):
    img = A.cutout(24, 40, 21)
    r, out = _run(tmp_path, img, "bc1a:0.5", "--mips", "--alpha-coverage", "128")
    assert r.returncode == 0, r.stderr
    d, got = _payload(itw, out)
    assert (d.width, d.height, d.mip_levels) == (40, 24, 6)
    ok, want = itw.compress_mipped("bc1a", img, alpha_coverage=128, settings=itw.Bc1aSettings(0.5))
    assert ok and np.array_equal(got, want)
    assert len([ln for ln in r.stdout.splitlines() if ln.startswith("coverage ")]) == 6


@pytest.mark.gpu
def test_single_image_with_flags_measured(itw, gpu, tmp_path):
    img = A.cutout(30, 41, 5)
    r, out = _run(tmp_path, img, "bc1a:0.25", "--bc-dither", "rgb,a", "--bc-uniform", "--measure")
    assert r.returncode == 0, r.stderr
    d, got = _payload(itw, out)
    assert (d.width, d.height, d.mip_levels) == (41, 30, 1)                              # a DirectXTex format: the image's own size
    ok, want = itw.compress_image("bc1a", img, settings=itw.Bc1aSettings(0.25, True, True, True))
    assert ok and np.array_equal(got, want)
    assert r.stdout.startswith("image 0: 41x30 bc1a psnr ")


@pytest.mark.parametrize("fmt,flags,word", [
    ("bc1", ("--bc-uniform",), "bc1a's flags"),
    ("bc3", ("--bc-dither", "a"), "bc1a's flags"),
    ("bc1a", ("--bc-dither", "b"), "--bc-dither takes"),
    ("bc1a", ("--normal", "normalize"), "not with --normal"),
    ("bc1a", ("--refine", "slow", "100"), "not with --normal or --refine"),
])
def test_flags_are_refused_where_they_mean_nothing(tmp_path, fmt, flags, word):
    r, out = _run(tmp_path, np.zeros((8, 8, 4), np.uint8), fmt, *flags)
    assert r.returncode == 2 and word in r.stderr and not out.exists(), (r.returncode, r.stderr)
