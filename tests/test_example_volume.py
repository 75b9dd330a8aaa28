"""examples/encode_dds with --volume: the raw input is depth slices of width x height, the file is the binding's volume DDS byte for
byte (compress_volume's payload behind itwDdsWriteHeader's volume header), and --decode reads it back in its own order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _mip3d as M3

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "encode_dds")


def _binding_file(itw, fmt, vol, levels, **options):
    d, h, w = vol.shape[:3]
    ok, blocks = itw.compress_volume(fmt, vol.copy(), levels=levels, **options)
    assert ok, itw.last_error()
    n = levels or M3.levels_of(w, h, d)
    parts, at = [], 0
    for *_, nb in itw.dds_volume_images(itw.DdsVolumeDesc(w, h, d, n, itw.DXGI_FORMAT[fmt])):
        parts.append(blocks[at:at + nb])
        at += nb
    assert at == blocks.size
    return itw.dds_volume_file(fmt, w, h, d, parts, n)


@pytest.mark.parametrize("name,fmt,half,size,args,levels,options", [
    ("bc1", "bc1", False, (12, 20, 6), ["--mips"], 0, dict()),
    ("bc1", "bc1", False, (16, 16, 8), ["--mips", "3"], 3, dict()),
    ("bc3", "bc3", False, (12, 20, 6), ["--mips", "--mip-filter", "cubic", "--mip-wrap", "uvw", "--srgb-mips"], 0, dict(filter="cubic", wrap="uvw", srgb=True)),
    ("bc4", "bc4", False, (5, 3, 7), ["--mips", "--mip-filter", "point"], 0, dict(filter="point")),
    ("bc2", "bc2", False, (8, 8, 4), ["--mips", "--mip-filter", "linear", "--mip-wrap", "w"], 0, dict(filter="linear", wrap="w")),
    ("bc7_ultrafast", "bc7", False, (8, 8, 4), [], 1, dict(profile="ultrafast")),
    ("bc6h_veryfast", "bc6h", True, (12, 20, 6), ["--mips", "--mip-filter", "triangle", "--mip-wrap", "vw"], 0, dict(profile="veryfast", filter="triangle", wrap="vw")),
])
def test_encode_dds_writes_the_bindings_volume_file_and_decodes_it(itw, gpu, tmp_path, name, fmt, half, size, args, levels, options):
    w, h, d = size
    vol = (M3.seeded_half_volume(d, h, w, 95) & 0x7FFF).astype(np.uint16) if half else M3.seeded_byte_volume(d, h, w, 95)
    raw, out, back = tmp_path / "in.raw", tmp_path / "out.dds", tmp_path / "back.raw"
    vol.tofile(raw)
    r = subprocess.run([EXE, "--volume", str(d)] + args + [name, str(w), str(h), str(raw), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, dtype=np.uint8)
    want = _binding_file(itw, fmt, vol, levels, **options)
    assert np.array_equal(got, want), (name, got.size, want.size)
    desc = itw.DdsDesc()
    assert itw.lib().itwDdsReadHeader(got.ctypes.data, got.size, C.byref(desc)) in (128, 148)
    assert (desc.width, desc.height, desc.array_size, desc.mip_levels, desc.is_cubemap) == (w, h, d, levels or M3.levels_of(w, h, d), itw.DDS_VOLUME)
    # --decode: every slice in file order, the lines name level and slice
    r = subprocess.run([EXE, "--decode", str(out), str(back)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    _, texels, amin = itw.load_dds_volume(got)
    assert np.array_equal(np.fromfile(back, dtype=np.uint8), np.concatenate([t.view(np.uint8).reshape(-1) for t in texels]))
    lines = r.stdout.strip().split("\n")
    rows = [(lh, lw, lv, sl) for lh, lw, lv, sl, _, _ in itw.dds_volume_images(desc)]
    assert lines == [f"image {i}: {lw} {lh} min_alpha {amin[i]} level {lv} slice {sl}" for i, (lh, lw, lv, sl) in enumerate(rows)]


def test_encode_dds_measures_a_volume_and_refuses_what_makes_no_sense_for_one(itw, gpu, tmp_path):
    w, h, d = 12, 20, 6
    vol = M3.seeded_byte_volume(d, h, w, 96)
    raw, out = tmp_path / "in.raw", tmp_path / "out.dds"
    vol.tofile(raw)
    r = subprocess.run([EXE, "--volume", str(d), "--mips", "--measure", "bc1", str(w), str(h), str(raw), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(out, dtype=np.uint8), _binding_file(itw, "bc1", vol, 0))
    chain = itw.generate_mips_3d(vol.copy())
    slices = [lv[z] for lv in chain for z in range(lv.shape[0])]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(slices) and all(ln.startswith(f"image {i}: {s.shape[1]}x{s.shape[0]} bc1 psnr ") for i, (ln, s) in enumerate(zip(lines, slices)))
    for bad, word in ((["--volume", "6", "--normal", "flipx"], "--volume does not go with"), (["--volume", "6", "--cube-cross"], "--volume does not go with"),
                      (["--volume", "6", "--mips", "--alpha-coverage", "128"], "--volume does not go with"), (["--volume", "6", "--resize", "8x8"], "--volume does not go with"),
                      (["--volume", "6", "--refine", "slow", "10"], "--volume does not go with"), (["--volume", "6", "--mip-filter", "cubic"], "with --mips"),
                      (["--volume", "6", "--srgb-mips"], "with --mips"), (["--volume", "0"], "depth of at least 1"), (["--volume", "6", "--mips", "9"], "has 5 levels"),
                      (["--volume", "7"], "cannot read"),
                      # point, linear and the w axis stay the volume's: without --volume the old messages
                      (["--mips", "--mip-filter", "point"], "--mip-filter takes cubic or triangle"), (["--mips", "--mip-wrap", "uvw"], "--mip-wrap takes u, v or uv")):
        r = subprocess.run([EXE] + bad + ["bc1", str(w), str(h), str(raw), str(tmp_path / "no.dds")], capture_output=True, text=True, timeout=300)
        assert r.returncode in (1, 2) and word in r.stderr and not (tmp_path / "no.dds").exists(), (bad, r.returncode, r.stderr)
    r = subprocess.run([EXE, "--volume", "6", "bc1", str(w), str(h), str(raw), str(tmp_path / "no.dds"), "4096"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--volume does not go with" in r.stderr
    # --preview takes a slice by its index in file order: slice 1 of level 1 is image 7, 6 x 10
    r = subprocess.run([EXE, "--preview", str(out), "7", str(tmp_path / "p.ppm"), "8", "8", "0", "0", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "image 7 (6x10)" in r.stderr, r.stderr
    r = subprocess.run([EXE, "--preview", str(out), "12", str(tmp_path / "q.ppm"), "8", "8", "0", "0", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "has no image 12" in r.stderr            # five levels of 6 + 3 + 1 + 1 + 1 = 12 slices, 0 .. 11
