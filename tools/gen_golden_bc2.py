"""Records the reference's BC2 streams into tests/golden/bc2_ref.npz: D3DXEncodeBC2 of oracle/_ref/libdxtex_bc_ref.so (tests/_dxtex_bc2.py
binds it) over the content the CPU and GPU tests share -- _dxtex_bc1's boundary_heavy (1 024 blocks) and strip (256 blocks) plus
_dxtex_bc2.alpha_blocks() (64 blocks) -- for the 8 flag combinations, five odd sizes with the partial-block fill, and D3DXDecodeBC2 of the decode tests' blocks.  The tests compare
the model, the kernel's text on the host and the GPU with these bytes, so they hold where the reference library is absent.
usage: python tools/gen_golden_bc2.py        (needs oracle/_ref, i.e. a build next to the reference tree)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _dxtex_bc2 as B2      # noqa: E402


def main():
    out = {}
    for name, img in B2.content().items():
        for flags in B2.FLAG_SETS:
            out[B2.golden_key(name, flags)] = B2.encode(img, flags)
    for h, w in B2.SIZES:                                   # partial blocks: DirectXTexCompress.cpp's {0, 0, 0, 1} fill
        for flags in B2.SIZE_FLAGS:
            out[B2.size_key(h, w, flags)] = B2.encode(B2.size_image(h, w), flags)
    out["decode.blocks"] = B2.decode_test_blocks()
    out["decode.ref"] = B2.decode(out["decode.blocks"])
    np.savez_compressed(B2.GOLDEN, **out)
    print("wrote", B2.GOLDEN, os.path.getsize(B2.GOLDEN), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
