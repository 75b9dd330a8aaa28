"""examples/encode_dds with --resize, --fit pow2 and --resize-filter: the image is fitted first and everything after sees the fitted image,
so the file's payload is what resize plus compress_mipped (tests/test_gpu_resize.py holds both against the model) predict."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _mip_filters as MF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "encode_dds")


def _payload(itw, path):
    f = np.fromfile(path, dtype=np.uint8)
    d = itw.DdsDesc()
    off = itw.lib().itwDdsReadHeader(f.ctypes.data, f.size, C.byref(d))
    assert off in (128, 148)
    return d, f[off:]


@pytest.mark.parametrize("args,size,options", [
    (["--resize", "33x20", "--resize-filter", "cubic"], (33, 20), dict(filter="cubic")),
    (["--resize", "64x16", "--resize-filter", "triangle", "--mip-wrap", "uv"], (64, 16), dict(filter="triangle", wrap="uv")),
    (["--resize", "20x12"], (20, 12), dict()),                       # exactly 2:1: the default's box
    (["--fit", "pow2"], (32, 16), dict()),
    (["--fit", "pow2", "--resize-filter", "point", "--srgb-mips"], (32, 16), dict(filter="point", srgb=True)),
])
def test_encode_dds_resizes_before_the_chain(itw, gpu, tmp_path, args, size, options):
    img = MF.seeded_byte_image(24, 40, 91)
    raw, out = tmp_path / "in.raw", tmp_path / "out.dds"
    img.tofile(raw)
    r = subprocess.run([EXE, "--mips"] + args + ["bc1", "40", "24", str(raw), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    d, got = _payload(itw, out)
    assert itw.fit_size(40, 24, "pow2") == (32, 16)
    assert (d.width, d.height, d.mip_levels) == (size[0], size[1], itw.mip_levels(*size))
    fitted = itw.resize(img.copy(), size=size, **options)
    chain_options = {k: v for k, v in options.items() if k in ("wrap", "srgb")}
    ok, want = itw.compress_mipped("bc1", fitted, **chain_options)
    ok2, same = itw.compress_mipped("bc1", img.copy(), resize=size, resize_filter=options.get("filter"), **chain_options)
    assert ok and ok2 and np.array_equal(got, want) and np.array_equal(same, want), (args, got.size, want.size)


def test_encode_dds_resizes_a_single_image_and_refuses_what_the_call_refuses(itw, gpu, tmp_path):
    img = MF.seeded_half_image(9, 14, 92)
    raw, out = tmp_path / "in.raw", tmp_path / "out.dds"
    img.tofile(raw)
    r = subprocess.run([EXE, "--resize", "28x12", "--resize-filter", "linear", "bc6h_veryfast", "14", "9", str(raw), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    d, got = _payload(itw, out)
    assert (d.width, d.height, d.mip_levels) == (28, 12, 1)
    fitted = itw.resize(img.copy(), size=(28, 12), filter="linear")
    ok, want = itw.compress_chain("bc6h", [fitted], settings=itw.bc6h_profile("veryfast"))
    assert ok and np.array_equal(got, np.asarray(want).reshape(-1))
    for bad, word in ((["--resize", "28x12", "--mip-wrap", "u", "--mips"], "linear filter with ITW_MIP_WRAP"), (["--resize-filter", "cubic"], "--resize WxH or --fit pow2"),
                      (["--resize", "28x12", "--fit", "pow2"], "one of the two"), (["--resize", "28x12", "--cube-cross"], "--cube-cross"), (["--resize", "0x4"], "WxH")):
        r = subprocess.run([EXE] + bad + ["bc6h_veryfast", "14", "9", str(raw), str(tmp_path / "no.dds")], capture_output=True, text=True, timeout=300)
        assert r.returncode in (1, 2) and word in r.stderr and not (tmp_path / "no.dds").exists(), (bad, r.returncode, r.stderr)
