"""Records the reference's signed BC6H decode into tests/golden/bc6hs_ref.npz: D3DXDecodeBC6HS of oracle/_ref/libdxtex_bc_ref.so
(tests/_dxtex_bc6hs.py binds it) over (a) the 8 192 blocks of _block_sweep.bc6h(), (b) the constructed blocks of every mode, (c) 4 096
random words and (d) D3DXEncodeBC6HS's stream of a 64 x 64 signed HDR surface.  The reference returns floats widened from halves; they are
narrowed back exactly (asserted) and stored as uint16 bits, RGB only: alpha is 1.0 in every texel, which is asserted here and not stored.
The tests compare the numpy model, the decoder's text on the host and the GPU with these bits, so they hold where the reference is absent.
usage: python tools/gen_golden_bc6hs.py        (needs oracle/_ref, i.e. a build next to the reference tree)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _dxtex_bc6hs as H      # noqa: E402


def main():
    sets = {"sweep": H.sweep_blocks(), "constructed": H.constructed_blocks(), "random": H.random_blocks(),
            "encoded": H.reference_encode(H.hdr_surface())}
    out = {}
    for name, blocks in sets.items():
        texels = H.reference_decode(blocks)
        assert (texels[..., 3] == 0x3C00).all()
        out[name + "_rgb"] = np.ascontiguousarray(texels[..., :3])
        if name != "sweep": out[name + "_blocks"] = np.ascontiguousarray(blocks, dtype=np.uint8)      # (the sweep is _block_sweep's own)
    np.savez_compressed(H.GOLDEN, **out)
    print("wrote", H.GOLDEN, os.path.getsize(H.GOLDEN), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
