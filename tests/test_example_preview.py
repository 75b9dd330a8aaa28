"""examples/encode_dds --preview <in.dds> <image index> <out.ppm> ...: the preview path through include/*.h alone -- header, itwDdsImage, one
itwPreviewBlocks -- against the binding (itw.preview) and the numpy restatement (tests/_preview.py), byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import _preview
from test_gpu_decode_chain import _want_image

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "encode_dds")


def _ppm(path):
    raw = open(path, "rb").read()
    magic, size, depth, body = raw.split(b"\n", 3)
    w, h = (int(v) for v in size.split())
    assert magic == b"P6" and depth == b"255" and len(body) == w * h * 3
    return np.frombuffer(body, dtype=np.uint8).reshape(h, w, 3)


def test_the_example_shows_images_of_a_mipped_file(itw, gpu, oracle, tmp_path):
    """A mipped bc7 DDS (52 x 36: 13 x 9 blocks, then 26 x 18, 13 x 9, ...) written by the library; image 0 magnified with alpha in byte 2, image 2
    minified from a negative offset."""
    import torch
    from itw_amd import surfaces
    top = surfaces.ldr_smooth(36, 52)                            # its alpha is a field of its own
    sizes = [(36, 52), (18, 26), (9, 13), (4, 6), (2, 3), (1, 1)]
    levels = [torch.from_numpy(np.ascontiguousarray(top[:h, :w])).to(gpu) for h, w in sizes]      # crops: any content will do
    ok, blocks = itw.compress_chain("bc7", levels, profile="alpha_veryfast")
    assert ok
    torch.cuda.synchronize()
    stream = blocks.cpu().numpy()
    nbs = [((w + 3) // 4) * ((h + 3) // 4) * 16 for h, w in sizes]
    offs = np.concatenate([[0], np.cumsum(nbs)])
    dds = tmp_path / "mips.dds"
    itw.dds_file("bc7", 52, 36, [stream[offs[i]:offs[i + 1]] for i in range(6)], mip_levels=6).tofile(dds)
    cases = [(0, dict(view_w=70, view_h=45, x=-6, y=-4, zoom=0.5, channels="rga", matte=0x102030)),
             (2, dict(view_w=21, view_h=17, x=-2, y=-3, zoom=2.5, channels="rgb", matte=0x0000FF))]
    for index, v in cases:
        h, w = sizes[index]
        ppm = tmp_path / f"view{index}.ppm"
        r = subprocess.run([EXE, "--preview", str(dds), str(index), str(ppm), str(v["view_w"]), str(v["view_h"]), str(v["x"]), str(v["y"]), repr(v["zoom"]),
                            v["channels"], "1.0", hex(v["matte"])], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got = _ppm(ppm)
        part = stream[offs[index]:offs[index + 1]]
        assert np.array_equal(got, itw.preview("bc7", part, w, h, **v)), index
        texels, _ = _want_image(oracle, "bc7", part, h, w)
        options = sum({"r": 4, "g": 8, "b": 16, "a": 32}[c] for c in v["channels"])
        assert np.array_equal(got, _preview.viewport(texels, v["view_w"], v["view_h"], v["x"], v["y"], v["zoom"], options, v["matte"])), index
    r = subprocess.run([EXE, "--preview", str(dds), "6", str(tmp_path / "none.ppm"), "8", "8", "0", "0", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "no image 6" in r.stderr
    r = subprocess.run([EXE, "--preview", str(dds), "0", str(tmp_path / "none.ppm"), "8", "8", "0", "0", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and not os.path.exists(tmp_path / "none.ppm")          # zoom 0 is refused
