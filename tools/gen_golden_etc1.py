"""Writes tests/golden/golden_etc1.npz: the ETC1 test input `ramp` and the SHA-256 of the input `noise` (tests/_etc1.py; noise is 16 KiB of
seeded random bytes that no compressor shortens: _etc1.load_golden regenerates it and checks the hash), the reference's block streams of both at
fastSkipTreshold 1, 6, 32 and 165 (oracle/_ref/libispc_texcomp_ref_full.so: the reference's kernel source as one scalar program
instance, made by build()), and beside each stream the RGB PSNR of its decoded image, decoded by the numpy decoder of tests/_etc1.py.
usage: python tools/gen_golden_etc1.py        (from the repository root, after build())"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _etc1  # noqa: E402

out = {}
for name, img in (("noise", _etc1.noise()), ("ramp", _etc1.ramp())):
    if name == "ramp":
        out[name] = img
    else:
        out[name + ".sha256"] = np.array(_etc1.sha256(img))
    for t in _etc1.GOLDEN_THRESHOLDS:
        stream = _etc1.ref_encode(img, t)
        texels, modes = _etc1.decode_np(stream, 64, 64)
        assert (modes >= 0).all()
        out[f"{name}.t{t}"] = stream
        out[f"{name}.t{t}.psnr"] = np.float64(_etc1.psnr_rgb(texels, img))
        print(name, t, f"{float(out[f'{name}.t{t}.psnr']):.3f} dB")
np.savez_compressed(_etc1.GOLDEN, **out)
print(_etc1.GOLDEN, os.path.getsize(_etc1.GOLDEN), "bytes")
