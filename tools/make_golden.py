"""Builds tests/golden/*.npz.  Run HERE (the build container): it reads the reference's sample images
from /root/reference/Sample Images (inputs only -- the reference ships no expected outputs), converts them to
the surface layouts the C ABI takes, and records the ORACLE's output for each (format, profile).

The golden outputs are written by the oracle; tests/test_reference_kernel_source.py then checks that the reference's own
kernel.ispc (built as a scalar program, oracle/_ref/libispc_texcomp_ref_full.so) emits the same bytes for every one of
them, so they are what the reference SOURCE produces under the pinned compiler / stdlib model.  They do not prove
equality with an ISPC binary (none can be built here: no ispc compiler) -- DESIGN.md section 5.

    python tools/make_golden.py            # writes inputs + golden block streams
"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import pyoracle  # noqa: E402
from itw_amd import surfaces  # noqa: E402
import rgbe  # noqa: E402

SAMPLES = "/root/reference/Sample Images"
OUT = os.path.join(ROOT, "tests", "golden")


def load_png_rgba(name):
    from PIL import Image
    im = Image.open(os.path.join(SAMPLES, name)).convert("RGBA")
    return np.ascontiguousarray(np.asarray(im, dtype=np.uint8))


def float_to_half_bits(rgb):
    """float32 -> half for the plugin's conversion (XMConvertFloatToHalf, IntelPlugin.cpp:343-366); alpha = 1.0.  IEEE 754 round to
    nearest even over every float, the project's pin (oracle/prepass.c).  The legacy DirectXMath software path
    departs from it, per sign, at 6 144 floats of the half-denormal range 0x33000001 .. 0x387fffff and at 4 095 floats of
    (65504, 65520) = 0x477fe001 .. 0x477fefff."""
    h = rgb.astype(np.float16).view(np.uint16)
    out = np.empty(rgb.shape[:2] + (4,), dtype=np.uint16)
    out[..., :3] = h
    out[..., 3] = 0x3C00
    return out


def pad4(img):
    """Edge replication to a multiple of 4 (the plugin's padding rule, IntelPlugin.cpp:893-928)."""
    h, w = img.shape[:2]
    return np.pad(img, ((0, (-h) % 4), (0, (-w) % 4), (0, 0)), mode="edge")


def main():
    os.makedirs(OUT, exist_ok=True)
    pyoracle.build()
    inputs = {
        "baboon": load_png_rgba("baboon.png"),                       # 256x256, alpha == 255  (BASELINE configs[0])
        "monkey": pad4(load_png_rgba("monkey.png")),                 # 220x220, real alpha
        "edge_cases": surfaces.ldr_edge_cases(),                     # 64x64 hand-picked block classes
    }
    hdr = {
        "monkey_hdr": pad4(float_to_half_bits(rgbe.read_hdr(os.path.join(SAMPLES, "monkey-32bit.hdr")))),
        "hdr_random_bits": surfaces.hdr_random_bits(32, 64),
    }
    np.savez_compressed(os.path.join(OUT, "inputs.npz"), **inputs, **hdr)
    gold = {}
    for name, img in inputs.items():
        for fmt in ("bc1", "bc3"):
            gold[f"{name}.{fmt}"] = pyoracle.encode(fmt, img)
        if pyoracle.has("oracle_CompressBlocksBC7"):
            profs = ["ultrafast", "veryfast", "fast", "basic", "slow",
                     "alpha_ultrafast", "alpha_veryfast", "alpha_fast", "alpha_basic", "alpha_slow"]
            for p in profs:
                if name == "baboon" and p not in ("veryfast", "basic", "slow", "alpha_basic"):
                    continue
                gold[f"{name}.bc7.{p}"] = pyoracle.encode("bc7", img, p)
    if pyoracle.has("oracle_CompressBlocksBC6H"):
        for name, img in hdr.items():
            for p in ("veryfast", "fast", "basic", "slow", "veryslow"):
                gold[f"{name}.bc6h.{p}"] = pyoracle.encode("bc6h", img, p)
    np.savez_compressed(os.path.join(OUT, "golden_blocks.npz"), **gold)
    for k, v in sorted(gold.items()):
        print(f"{k:40s} {v.size:8d} B  sha256 {surfaces.sha256(v)[:16]}")


def main_bc45():
    """BC4/BC5 (the DirectXTex formats): separate file so the ISPC-format fixtures stay byte-identical.  Includes the
    217 x 215 and 5 x 7 crops of monkey.png (odd sizes: DirectXTex's partial-block rule on both edges)."""
    pyoracle.build()
    monkey = load_png_rgba("monkey.png")
    data = {"monkey_crop.input": np.ascontiguousarray(monkey[1:218, 2:217]),
            "tiny.input": np.ascontiguousarray(monkey[40:45, 60:67])}
    cases = {"baboon": load_png_rgba("baboon.png"), "edge_cases": surfaces.ldr_edge_cases(),
             "monkey_crop": data["monkey_crop.input"], "tiny": data["tiny.input"]}
    for name, img in cases.items():
        for fmt in ("bc4", "bc5"):
            data[f"{name}.{fmt}"] = pyoracle.encode_bc45(fmt, img)
    np.savez_compressed(os.path.join(OUT, "golden_bc45.npz"), **data)
    for k, v in sorted(data.items()):
        print(f"{k:40s} {v.size:8d} B  sha256 {surfaces.sha256(v)[:16]}")


def main_samples2():
    """More of the reference's sample images (inputs committed as tests/golden/samples2.npz) and the full-size I2 surface
    (`colors-16M.png`, regenerated by surfaces.colors_16m()): the ORACLE's output of every format / profile is recorded as
    a SHA-256 only (tests/golden/samples2_sha256.json) -- whole-stream pins for the CPU and GPU suites."""
    import json
    pyoracle.build()
    i2 = surfaces.colors_16m()
    assert np.array_equal(i2, load_png_rgba("colors-16M.png")) and surfaces.sha256(i2) == surfaces.COLORS_16M_SHA256
    ldr = {"colors260k": load_png_rgba("colors-260K.png"), "gradients": load_png_rgba("gradients.png"),
           "normals": load_png_rgba("normals.png"), "radial": load_png_rgba("radial-grayscale.png"),
           "test_a": load_png_rgba("test-a.png"), "landscape_detail": load_png_rgba("landscape-detail.jpg")}
    hdr = {"hdr_probe": pad4(float_to_half_bits(rgbe.read_hdr(os.path.join(SAMPLES, "HDR.hdr"))))}
    np.savez_compressed(os.path.join(OUT, "samples2.npz"), **ldr, **hdr)
    sha = {}
    bc7 = ["ultrafast", "veryfast", "fast", "basic", "slow", "alpha_ultrafast", "alpha_veryfast", "alpha_fast", "alpha_basic", "alpha_slow"]
    for name, raw in ldr.items():
        img = pad4(raw)                                               # what the plugin hands to the ISPC formats
        for fmt in ("bc1", "bc3"):
            sha[f"{name}.{fmt}"] = surfaces.sha256(pyoracle.encode(fmt, img))
        for fmt in ("bc4", "bc5"):
            sha[f"{name}.{fmt}"] = surfaces.sha256(pyoracle.encode_bc45(fmt, raw))      # unpadded: DirectXTex's own rule
        for p in bc7:
            sha[f"{name}.bc7.{p}"] = surfaces.sha256(pyoracle.encode("bc7", img, p))
    for name, img in hdr.items():
        for p in ("veryfast", "fast", "basic", "slow", "veryslow"):
            sha[f"{name}.bc6h.{p}"] = surfaces.sha256(pyoracle.encode("bc6h", img, p))
    for fmt in ("bc1", "bc3", "bc4", "bc5"):
        sha[f"colors16m.{fmt}"] = surfaces.sha256(pyoracle.encode_mt(fmt, i2))
    for p in ("basic", "slow", "alpha_basic"):
        sha[f"colors16m.bc7.{p}"] = surfaces.sha256(pyoracle.encode_mt("bc7", i2, p))
        print("colors16m bc7", p, "done", flush=True)
    with open(os.path.join(OUT, "samples2_sha256.json"), "w") as f:
        json.dump(sha, f, indent=1, sort_keys=True)
    print(len(sha), "streams pinned")


if __name__ == "__main__":
    if "--samples2" in sys.argv:
        main_samples2()
    elif "--bc45" in sys.argv:
        main_bc45()
    else:
        main()
