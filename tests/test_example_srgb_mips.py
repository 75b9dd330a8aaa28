"""examples/encode_dds.cpp --mips --srgb-mips: the mipped DDS's payload is the binding's compress_mipped(srgb=True), which is not the plain
chain's; the option is refused where it has no meaning."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "encode_dds")


def _run(tmp_path, img, fmt, *flags):
    raw, out = tmp_path / "in.raw", tmp_path / "out.bin"
    np.ascontiguousarray(img).tofile(raw)
    h, w = img.shape[:2]
    return subprocess.run([EXE, *flags, fmt, str(w), str(h), str(raw), str(out)], capture_output=True, text=True, timeout=300), out


@pytest.mark.gpu
def test_srgb_mips_writes_the_payload_of_the_python_path(itw, gpu, tmp_path):
    img = np.random.default_rng(11).integers(0, 256, (24, 40, 4), dtype=np.uint8)
    r, out = _run(tmp_path, img, "bc7_veryfast", "--mips", "--srgb-mips")
    assert r.returncode == 0, r.stderr
    f = np.fromfile(out, dtype=np.uint8)
    d = itw.DdsDesc()
    off = itw.lib().itwDdsReadHeader(f.ctypes.data, f.size, C.byref(d))
    assert off in (128, 148) and d.dxgi_format == 98 and (d.width, d.height, d.mip_levels) == (40, 24, 6)
    ok, want = itw.compress_mipped("bc7", img, profile="veryfast", srgb=True)
    ok2, plain = itw.compress_mipped("bc7", img, profile="veryfast")
    assert ok and ok2 and f.size == off + want.size and np.array_equal(f[off:], want) and not np.array_equal(want, plain)


@pytest.mark.gpu
def test_srgb_mips_of_a_cube_cross(itw, gpu, tmp_path):
    img = np.random.default_rng(12).integers(0, 256, (48, 64, 4), dtype=np.uint8)           # faces of 16 x 16
    r, out = _run(tmp_path, img, "bc1", "--cube-cross", "--mips", "3", "--srgb-mips")
    assert r.returncode == 0, r.stderr
    f = np.fromfile(out, dtype=np.uint8)
    faces = [np.ascontiguousarray(v) for v in itw.cube_cross_faces(img)]
    ok, want = itw.compress_mipped("bc1", faces, levels=3, srgb=True)
    assert ok and np.array_equal(f[f.size - want.size:], want)


@pytest.mark.parametrize("fmt,flags,code", [("bc1", ("--srgb-mips",), 2), ("bc5_snorm", ("--mips", "--srgb-mips", "--signed-normal", "int8"), 2),
                                            ("bc6h_veryfast", ("--mips", "--srgb-mips"), 1), ("bc5", ("--mips", "--srgb-mips", "--normal", "normalize"), 1)])
def test_srgb_mips_is_refused_where_it_means_nothing(tmp_path, fmt, flags, code):
    """Without --mips and with a signed source the program refuses; RGBA16F formats and normal maps are refused by the library, before any
    device work, so this needs no GPU."""
    img = np.zeros((8, 8, 4), np.uint16 if fmt.startswith("bc6h") else np.uint8)
    r, out = _run(tmp_path, img, fmt, *flags)
    assert r.returncode == code and "srgb" in r.stderr.lower() and not out.exists(), (r.returncode, r.stderr)
