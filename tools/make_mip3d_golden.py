#!/usr/bin/env python3
"""Records tests/golden/mip3d_ref.npz and mip3d_ref_sha256.json: the outputs of the REFERENCE'S OWN _Generate3DMipsPointFilter,
_Generate3DMipsBoxFilter, _Generate3DMipsLinearFilter, _Generate3DMipsCubicFilter and _Generate3DMipsTriangleFilter
(DirectXTexMipmaps.cpp) on seeded RGBA16F volumes.  Run by hand, never by build() or a test:

    python tools/make_mip3d_golden.py REFERENCE_ROOT [WORK_DIR]

Nothing of the reference is in this file.  At run time it cuts the five function bodies out of DirectXTexMipmaps.cpp (from the point
filter's first line to the entry points' banner) and, out of Filters.h, everything from the box helpers to the end of the TriangleFilter
namespace, writes them into WORK_DIR next to the harness, and compiles the lot over oracle/ref_build/dxmath_stub with -O1
-ffp-contract=off.  The glue -- the vector operators, the RGBA16F scanline reading, the point filter's scanline functions -- is the text of
tools/make_mipfilter_golden.py and tools/make_resize_golden.py, taken from those modules; this file adds a volume image (slices in
level-major order, GetImage(level, item, slice)) under the name the cut text uses, ispow2, the W bits of TEX_FILTER, and a main().

Cases and names are tests/_mip3d.py's: every volume under every filter that accepts it (box: powers of two only, as the reference
refuses the rest), cubic and triangle under clamp, wrap W and wrap UVW; two wide volumes under box, where only the levels whose source
height is at least 2 are recorded (below them the reference reads a stale scanline, the library's one stated divergence).  Target storage
starts as 0xEE.  Small cases go into the npz whole, level by level as (d, h, w, 4) half bits; every case as SHA-256 of its input and of
its recorded levels, concatenated.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _mip3d as M3  # noqa: E402
import make_mipfilter_golden as MG  # noqa: E402
import make_resize_golden as RG  # noqa: E402

GLUE = RG.HARNESS.split('#include "cut_filters.inc"')[0]
HARNESS = GLUE + r"""
/* glue of this tool: a volume chain of plain arrays, its slices level-major, under the name the cut text uses */
enum { TEX_FILTER_WRAP_W = 0x4, TEX_FILTER_MIRROR_W = 0x40 };
inline bool ispow2(size_t x) { return x && !(x & (x - 1)); }
struct VolumeChain {
    TexMetadata meta; std::vector<Image> images; std::vector<size_t> first;      /* first[l]: index of level l's slice 0 */
    const Image* GetImages() const { return images.data(); }
    const TexMetadata& GetMetadata() const { return meta; }
    const Image* GetImage(size_t level, size_t, size_t slice) const { return &images[first[level] + slice]; }
};
#define ScratchImage VolumeChain

#include "cut_filters.inc"
#include "cut_mipmaps3d.inc"
} // namespace DirectX

using namespace DirectX;

/* mip3d_ref point|box|linear|cubic|triangle FILTERBITS W H D in.bin out.bin: every level below the base, slices in order */
int main(int argc, char** argv)
{
    if (argc != 8) return 2;
    const DWORD filter = (DWORD)strtoul(argv[2], 0, 0);
    const size_t w = strtoul(argv[3], 0, 10), h = strtoul(argv[4], 0, 10), d = strtoul(argv[5], 0, 10);
    size_t levels = 1;
    for (size_t m = std::max(w, std::max(h, d)); m > 1; m >>= 1) levels++;
    VolumeChain chain;
    chain.meta.width = w; chain.meta.height = h;
    std::vector<std::vector<uint8_t>> store;
    for (size_t l = 0; l < levels; l++) {
        const size_t lw = (w >> l) ? (w >> l) : 1, lh = (h >> l) ? (h >> l) : 1, ld = (d >> l) ? (d >> l) : 1;
        chain.first.push_back(store.size());
        for (size_t z = 0; z < ld; z++) store.emplace_back(lw * lh * 8, (uint8_t)0xEE);
    }
    for (size_t l = 0, i = 0; l < levels; l++) {
        const size_t lw = (w >> l) ? (w >> l) : 1, lh = (h >> l) ? (h >> l) : 1, ld = (d >> l) ? (d >> l) : 1;
        for (size_t z = 0; z < ld; z++, i++) chain.images.push_back(Image{lw, lh, DXGI_FORMAT_R16G16B16A16_FLOAT, lw * 8, store[i].data()});
    }
    FILE* f = fopen(argv[6], "rb");
    if (!f) return 3;
    for (size_t z = 0; z < d; z++) if (fread(store[z].data(), 1, store[z].size(), f) != store[z].size()) return 3;
    fclose(f);
    if (levels > 1) {
        HRESULT hr = E_INVALIDARG;
        if (!strcmp(argv[1], "point")) hr = _Generate3DMipsPointFilter(d, levels, chain);
        else if (!strcmp(argv[1], "box")) hr = _Generate3DMipsBoxFilter(d, levels, filter, chain);
        else if (!strcmp(argv[1], "linear")) hr = _Generate3DMipsLinearFilter(d, levels, filter, chain);
        else if (!strcmp(argv[1], "cubic")) hr = _Generate3DMipsCubicFilter(d, levels, filter, chain);
        else if (!strcmp(argv[1], "triangle")) hr = _Generate3DMipsTriangleFilter(d, levels, filter, chain);
        if (hr != S_OK) return 4;
    }
    f = fopen(argv[7], "wb");
    for (size_t i = d; i < store.size(); i++) fwrite(store[i].data(), 1, store[i].size(), f);
    fclose(f);
    return 0;
}
"""

SMALL = 16 * 16 * 16      # texels of the base up to which a case is stored whole


def build(ref_root, work):
    dxtex = os.path.join(ref_root, "3rdParty", "DirectXTex", "DirectXTex")
    with open(os.path.join(dxtex, "Filters.h"), encoding="latin-1") as f:
        fl = f.readlines()
    with open(os.path.join(dxtex, "DirectXTexMipmaps.cpp"), encoding="latin-1") as f:
        ml = f.readlines()
    filters = MG.cut(fl, "g_boxScale =", "// Triangle filtering helpers") + MG.cut(fl, "namespace TriangleFilter", "}; // namespace") + ["}\n"]
    mipmaps = MG.cut(ml, "static HRESULT _Generate3DMipsPointFilter(", "// Entry-points")
    with open(os.path.join(work, "cut_filters.inc"), "w") as f:
        f.writelines(filters)
    with open(os.path.join(work, "cut_mipmaps3d.inc"), "w") as f:
        f.writelines(mipmaps)
    with open(os.path.join(work, "harness.cpp"), "w") as f:
        f.write(HARNESS)
    exe = os.path.join(work, "mip3d_ref")
    subprocess.run(["g++", "-std=c++17", "-O1", "-w", "-ffp-contract=off", "-I", os.path.join(ROOT, "oracle", "ref_build", "dxmath_stub"), "-I", work,
                    os.path.join(work, "harness.cpp"), "-o", exe], check=True)
    return exe


def run_chain(exe, work, filt, wrap, base):
    d, h, w = base.shape[:3]
    src, dst = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
    np.ascontiguousarray(base).tofile(src)
    bits = (1 if "u" in wrap else 0) | (2 if "v" in wrap else 0) | (4 if "w" in wrap else 0)             # TEX_FILTER_WRAP_U / _V / _W
    subprocess.run([exe, filt, str(bits), str(w), str(h), str(d), src, dst], check=True)
    flat = np.fromfile(dst, dtype=np.uint16)
    out, at = [], 0
    for l in range(1, M3.levels_of(w, h, d)):
        lw, lh, ld = M3.level_size(w, h, d, l)
        out.append(flat[at:at + ld * lh * lw * 4].reshape(ld, lh, lw, 4))
        at += ld * lh * lw * 4
    assert at == flat.size
    return out


def main():
    ref_root = sys.argv[1]
    work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="mip3d_ref_")
    os.makedirs(work, exist_ok=True)
    exe = build(ref_root, work)
    arrays, pins = {}, {"cases": {}}
    todo = [(c, True, M3.variants(*c[:3])) for c in M3.CASES] + [(c, False, M3.variants(*c[:3])) for c in M3.SHA_CASES] \
        + [(c, True, [("box", "")]) for c in M3.WIDE_BOX_CASES]
    for (w, h, d, seed), whole, variants in todo:
        base = M3.seeded_half_volume(d, h, w, seed)
        stored = whole and w * h * d <= SMALL
        if stored:
            arrays[f"in_{w}x{h}x{d}"] = base
        for filt, wrap in variants:
            levels = run_chain(exe, work, filt, wrap, base)
            keep = M3.recorded_levels(filt, w, h, d)
            name = M3.case_name(filt, wrap, w, h, d)
            pins["cases"][name] = {"filter": filt, "wrap": wrap, "width": w, "height": h, "depth": d, "seed": seed, "stored": stored, "levels": keep,
                                   "input_sha256": hashlib.sha256(base.tobytes()).hexdigest(),
                                   "levels_sha256": hashlib.sha256(b"".join(np.ascontiguousarray(levels[l - 1]).tobytes() for l in keep)).hexdigest()}
            if stored:
                for l in keep:
                    arrays[f"{name}_l{l}"] = levels[l - 1]
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "mip3d_ref.npz"), **arrays)
    with open(os.path.join(gold, "mip3d_ref_sha256.json"), "w") as f:
        json.dump(pins, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(pins["cases"]), "cases ->", gold, os.path.getsize(os.path.join(gold, "mip3d_ref.npz")), "bytes")


if __name__ == "__main__":
    main()
