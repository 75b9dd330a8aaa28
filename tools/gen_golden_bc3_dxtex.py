"""Records the reference's BC3 streams into tests/golden/bc3_dxtex_ref.npz: D3DXEncodeBC3 of oracle/_ref/libdxtex_bc_ref.so
(tests/_dxtex_bc3.py binds it) over the content the CPU and GPU tests share -- _dxtex_bc1's boundary_heavy (1 024 blocks) and strip (256
blocks) plus _dxtex_bc3.alpha_blocks() (128 blocks) -- for the 8 flag combinations, and _dxtex_bc2's five odd sizes with the partial-block
fill under its SIZE_FLAGS.  Before it records, it checks that the numpy model reads every stream as the reference wrote it and that the
branches the tests ask for are taken (tests/test_bc3_dxtex_cpu.py asserts the same of the recording).  The tests compare the model, the
kernel's text on the host and the GPU with these bytes, so they hold where the reference library is absent.
usage: python tools/gen_golden_bc3_dxtex.py        (needs oracle/_ref, i.e. a build next to the reference tree)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _dxtex_bc3 as B3      # noqa: E402
from _dxtex_snorm import block_texels      # noqa: E402


def main():
    out = {}
    taken = {k: 0 for k in B3.BRANCHES + B3.DITHER_A_BRANCHES}
    for name, img in B3.content().items():
        for flags in B3.FLAG_SETS:
            stream = B3.encode(img, flags)
            blocks, branches, _ = B3.model(block_texels(img), flags)
            assert np.array_equal(blocks.reshape(-1), stream), (name, hex(flags))
            for k, v in B3.census(branches).items():
                taken[k] += v
            out[B3.golden_key(name, flags)] = stream
    missing = [k for k, v in taken.items() if not v and k not in B3.UNREACHED_BRANCHES]
    assert not missing, missing
    print("branches taken:", taken)
    for h, w in B3.SIZES:                                   # partial blocks: DirectXTexCompress.cpp's {0, 0, 0, 1} fill
        for flags in B3.SIZE_FLAGS:
            out[B3.size_key(h, w, flags)] = B3.encode(B3.size_image(h, w), flags)
    np.savez_compressed(B3.GOLDEN, **out)
    print("wrote", B3.GOLDEN, os.path.getsize(B3.GOLDEN), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
