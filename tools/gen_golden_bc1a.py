"""Records the reference's BC1-with-1-bit-alpha streams into tests/golden/bc1a_ref.npz: D3DXEncodeBC1 of oracle/_ref/libdxtex_bc_ref.so
(tests/_dxtex_bc1.py binds it) over the content the CPU and GPU tests share -- boundary_heavy (1 024 blocks) and the constructed strip
(256 blocks) -- for the 8 flag combinations x 5 alpha_ref values.  The
tests compare the model, the kernel's text on the host and the GPU with these bytes, so they hold where the reference library is absent.
usage: python tools/gen_golden_bc1a.py        (needs oracle/_ref, i.e. a build next to the reference tree)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _dxtex_bc1 as B      # noqa: E402


def main():
    out = {}
    for name, img in B.content().items():
        for ref in B.ALPHA_REFS:
            for flags in B.FLAG_SETS:
                out[B.golden_key(name, ref, flags)] = B.encode(img, ref, flags)
    np.savez_compressed(B.GOLDEN, **out)
    print("wrote", B.GOLDEN, os.path.getsize(B.GOLDEN), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
