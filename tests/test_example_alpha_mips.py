"""examples/encode_dds.cpp --mips --alpha-weight --alpha-coverage <ref>: the mipped DDS's payload is the binding's
compress_mipped(alpha_weight=True, alpha_coverage=ref), the report lines are the model's rows, and the options are refused where the call
refuses them."""
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


@pytest.mark.gpu
def test_alpha_mips_write_the_payload_of_the_python_path(itw, gpu, tmp_path):
    img = A.cutout(24, 40, 21)
    r, out = _run(tmp_path, img, "bc3", "--mips", "--alpha-coverage", "128", "--alpha-weight")
    assert r.returncode == 0, r.stderr
    f = np.fromfile(out, dtype=np.uint8)
    d = itw.DdsDesc()
    off = itw.lib().itwDdsReadHeader(f.ctypes.data, f.size, C.byref(d))
    assert off in (128, 148) and (d.width, d.height, d.mip_levels) == (40, 24, 6)
    ok, want = itw.compress_mipped("bc3", img, alpha_weight=True, alpha_coverage=128)
    ok2, plain = itw.compress_mipped("bc3", img)
    assert ok and ok2 and f.size == off + want.size and np.array_equal(f[off:], want) and not np.array_equal(want, plain)
    _, rows = A.chain(img, weight=True, ref=128)
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("coverage ")]
    assert [(int(p[2]), int(p[4])) for p in lines] == [(0, l) for l in range(6)]
    assert [(int(p[6]), int(p[8]), int(p[10]), int(p[12])) for p in lines] == rows


@pytest.mark.parametrize("fmt,flags,code,word", [
    ("bc3", ("--alpha-weight",), 2, "--mips"),
    ("bc5", ("--mips", "--alpha-coverage", "128", "--normal", "normalize"), 2, "--normal"),
    ("bc5_snorm", ("--mips", "--alpha-weight", "--signed-normal", "int8"), 2, "--signed-normal"),
    ("bc6h_veryfast", ("--mips", "--alpha-weight"), 1, "DXGI format 95"),
    ("bc5_snorm", ("--mips", "--alpha-coverage", "128"), 1, "DXGI format 84"),
    ("bc3", ("--mips", "--alpha-coverage", "256"), 1, "coverage_ref"),
])
def test_the_alpha_options_are_refused_where_the_call_refuses_them(tmp_path, fmt, flags, code, word):
    """The program refuses what has no --mips, a normal map or a signed source; the library refuses the rest before any device work, so
    this needs no GPU."""
    img = np.zeros((8, 8, 4), np.uint16 if fmt.startswith("bc6h") else np.uint8)
    r, out = _run(tmp_path, img, fmt, *flags)
    assert r.returncode == code and word in r.stderr and not out.exists(), (r.returncode, r.stderr)
