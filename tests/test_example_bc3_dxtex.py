"""examples/encode_dds.cpp with the format bc3_dxtex: the file is what Python builds from the reference's recorded streams
(tests/golden/bc3_dxtex_ref.npz) -- a DXT5 file, byte for byte --, --decode reads it back, and the flags are refused where they have no
meaning."""
import os
import subprocess

import numpy as np
import pytest

import _dxtex_bc3 as B3
from _dxtex_bc2 import cutout
from _dxtex_snorm import block_texels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "encode_dds")


def _run(tmp_path, img, fmt, *flags):
    raw, out = tmp_path / "in.raw", tmp_path / "out.dds"
    np.ascontiguousarray(img).tofile(raw)
    h, w = img.shape[:2]
    return subprocess.run([EXE, *flags, fmt, str(w), str(h), str(raw), str(out)], capture_output=True, text=True, timeout=300), out


@pytest.mark.parametrize("fmt,flags,word", [
    ("bc3_dxtex", ("--bc-dither", "b"), "--bc-dither takes"),
    ("bc3_dxtex", ("--normal", "normalize"), "not with --normal"),
    ("bc3_dxtex", ("--refine", "slow", "100"), "not with --normal or --refine"),
    ("bc3_dxtex:0.5", (), "unknown format"),
    ("bc3", ("--bc-dither", "a"), "bc3_dxtex's"),
])
def test_flags_are_refused_where_they_mean_nothing(tmp_path, fmt, flags, word):
    r, out = _run(tmp_path, np.zeros((8, 8, 4), np.uint8), fmt, *flags)
    assert r.returncode == 2 and word in r.stderr and not out.exists(), (r.returncode, r.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("args,flags", [((), 0), (("--bc-dither", "a"), B3.DITHER_A), (("--bc-dither", "rgb,a", "--bc-uniform"), B3.DITHER_RGB | B3.DITHER_A | B3.UNIFORM)],
                         ids=["plain", "dither_a", "all_flags"])
def test_single_image_is_the_file_of_the_recorded_stream_and_decodes_back(itw, gpu, tmp_path, args, flags):
    img = B3.content()["strip"]                                                          # 128 x 32
    r, out = _run(tmp_path, img, "bc3_dxtex", *args, "--measure")
    assert r.returncode == 0, r.stderr
    want = B3.golden()[B3.golden_key("strip", flags)]
    got = np.fromfile(out, dtype=np.uint8)
    assert got[84:88].tobytes() == b"DXT5" and np.array_equal(got, itw.dds_file("bc3_dxtex", 128, 32, [want]))
    assert r.stdout.startswith("image 0: 128x32 bc3_dxtex psnr ")
    back = tmp_path / "back.raw"
    r = subprocess.run([EXE, "--decode", str(out), str(back)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    texels = np.fromfile(back, dtype=np.uint8).reshape(32, 128, 4)
    assert np.array_equal(texels, itw.decode_image("bc3", want, (32, 128)))
    assert r.stdout.startswith("image 0: 128 32 min_alpha %d" % int(texels[..., 3].min()))


@pytest.mark.gpu
def test_an_odd_size_keeps_its_partial_blocks(itw, gpu, tmp_path):
    img = B3.size_image(61, 75)
    r, out = _run(tmp_path, img, "bc3_dxtex", "--bc-dither", "rgb,a")
    assert r.returncode == 0, r.stderr
    want = B3.golden()[B3.size_key(61, 75, B3.DITHER_RGB | B3.DITHER_A)]
    assert np.array_equal(np.fromfile(out, dtype=np.uint8), itw.dds_file("bc3_dxtex", 75, 61, [want]))


@pytest.mark.gpu
def test_mipped_cutout_writes_the_references_stream_of_every_generated_level(itw, gpu, tmp_path):
    img = cutout(24, 40, 21)
    r, out = _run(tmp_path, img, "bc3_dxtex", "--mips", "--alpha-coverage", "128", "--bc-dither", "a")
    assert r.returncode == 0, r.stderr
    chain = itw.generate_mips(img, alpha_coverage=128)
    assert len(chain) == 6
    levels = [B3.model(block_texels(np.ascontiguousarray(lv)), B3.DITHER_A)[0].reshape(-1) for lv in chain]
    assert np.array_equal(np.fromfile(out, dtype=np.uint8), itw.dds_file("bc3_dxtex", 40, 24, levels, mip_levels=6))
    back = tmp_path / "back.raw"
    r = subprocess.run([EXE, "--decode", str(out), str(back)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and len(r.stdout.splitlines()) == 6, r.stdout + r.stderr
