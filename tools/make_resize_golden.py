#!/usr/bin/env python3
"""Records tests/golden/resize_ref.npz and resize_ref_sha256.json: the outputs of the REFERENCE'S OWN _ResizePointFilter, _ResizeBoxFilter,
_ResizeLinearFilter, _ResizeCubicFilter and _ResizeTriangleFilter (DirectXTexResize.cpp) and of _CreateLinearFilter, _CreateCubicFilter and
TriangleFilter::_Create (Filters.h) on seeded RGBA16F images, between free (source, target) sizes.  Run by hand, never by build() or a test:

    python tools/make_resize_golden.py REFERENCE_ROOT [WORK_DIR]

Nothing of the reference is in this file.  At run time it cuts the five function bodies out of DirectXTexResize.cpp and, out of Filters.h,
the box helpers (g_boxScale, AVERAGE4), the linear helpers (LinearFilter, _CreateLinearFilter, BILINEAR_INTERPOLATE) and the pieces
tools/make_mipfilter_golden.py cuts (the cubic helpers, the TriangleFilter namespace), writes them into WORK_DIR next to the harness, and
compiles the lot over oracle/ref_build/dxmath_stub with -O1 -ffp-contract=off.  The glue -- plain-array images, the vector operators, the
RGBA16F scanline reading -- is make_mipfilter_golden.py's own text, taken from that module; this file adds the scalar-times-vector
operators BILINEAR_INTERPOLATE uses, the point filter's _LoadScanline / _StoreScanline (the same two functions without the filter
argument) and a main().

A case is a list of sizes: two for a resize, more for a chain whose level l is filtered from level l-1 as stored.  Each is recorded under
every filter that accepts it -- box at exactly 2:1 only -- and under clamp, wrap U, wrap V and wrap UV; cubic also under mirror UV; linear
not where the library refuses it (a wrap bit on an axis with dest >= source > 1).  Target storage starts as zeros, so a triangle
destination row that no list entry reaches reads as the zeros the library writes there.  Levels of at most SMALL texels go into the npz
whole, every case as SHA-256 of its input and of its concatenated levels.  The per-axis tables of every (source, dest) pair the cases
hold are recorded likewise; the json also counts, per triangle table, the destinations no entry reaches.
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
import _mip_filters as MF  # noqa: E402
import _resize as R  # noqa: E402
import make_mipfilter_golden as MG  # noqa: E402

SMALL = 4096          # texels of a level up to which it is stored whole

GLUE = MG.HARNESS.split('#include "cut_filters.inc"')[0]
HARNESS = GLUE + r"""
/* glue of this tool: a vector times a scalar, either way round, one fp32 multiply per lane */
inline XMVECTOR operator*(FXMVECTOR v, float s) { return XMVectorMultiply(v, XMVectorReplicate(s)); }
inline XMVECTOR operator*(float s, FXMVECTOR v) { return XMVectorMultiply(XMVectorReplicate(s), v); }
/* the point filter's scanline functions: the same two without the filter argument */
static bool _LoadScanline(XMVECTOR* dst, size_t count, const uint8_t* src, size_t size, DXGI_FORMAT f) { return _LoadScanlineLinear(dst, count, src, size, f, 0); }
static bool _StoreScanline(void* dst, size_t size, DXGI_FORMAT f, XMVECTOR* src, size_t count) { return _StoreScanlineLinear(dst, size, f, src, count, 0); }

#include "cut_filters.inc"
#include "cut_resize.inc"
} // namespace DirectX

using namespace DirectX;

/* resize_ref point|box|linear|cubic|triangle FILTERBITS SW SH DW DH in.bin out.bin
   resize_ref lineartable|cubictable|triangletable ADDRESS SOURCE DEST out.bin      (ADDRESS 0 clamp, 1 wrap, 2 mirror) */
int main(int argc, char** argv)
{
    if (argc == 6) {
        const int address = atoi(argv[2]);
        const size_t source = strtoul(argv[3], 0, 10), dest = strtoul(argv[4], 0, 10);
        FILE* f = fopen(argv[5], "wb");
        if (!strcmp(argv[1], "lineartable")) {
            std::vector<LinearFilter> lf(dest);
            _CreateLinearFilter(source, dest, address == 1, lf.data());
            for (size_t i = 0; i < dest; i++) {
                const int32_t u[2] = {(int32_t)lf[i].u0, (int32_t)lf[i].u1};
                const float w[2] = {lf[i].weight0, lf[i].weight1};
                fwrite(u, 4, 2, f); fwrite(w, 4, 2, f);
            }
        } else if (!strcmp(argv[1], "cubictable")) {
            std::vector<CubicFilter> cf(dest);
            _CreateCubicFilter(source, dest, address == 1, address == 2, cf.data());
            for (size_t i = 0; i < dest; i++) {
                const int32_t u[4] = {(int32_t)cf[i].u0, (int32_t)cf[i].u1, (int32_t)cf[i].u2, (int32_t)cf[i].u3};
                fwrite(u, 4, 4, f); fwrite(&cf[i].x, 4, 1, f);
            }
        } else if (!strcmp(argv[1], "triangletable")) {
            std::unique_ptr<TriangleFilter::Filter> tf;
            if (TriangleFilter::_Create(source, dest, address == 1, tf) != S_OK) return 5;
            const uint8_t* p = reinterpret_cast<const uint8_t*>(tf->from);
            const uint8_t* end = reinterpret_cast<const uint8_t*>(tf.get()) + tf->sizeInBytes;
            for (size_t u = 0; p < end; u++) {
                const TriangleFilter::FilterFrom* from = reinterpret_cast<const TriangleFilter::FilterFrom*>(p);
                for (size_t j = 0; j < from->count; j++) {
                    const int32_t idx[2] = {(int32_t)u, (int32_t)from->to[j].u};
                    fwrite(idx, 4, 2, f); fwrite(&from->to[j].weight, 4, 1, f);
                }
                p += from->sizeInBytes;
            }
        } else return 2;
        fclose(f);
        return 0;
    }
    if (argc != 9) return 2;
    const DWORD filter = (DWORD)strtoul(argv[2], 0, 0);
    const size_t sw = strtoul(argv[3], 0, 10), sh = strtoul(argv[4], 0, 10), dw = strtoul(argv[5], 0, 10), dh = strtoul(argv[6], 0, 10);
    std::vector<uint8_t> in(sw * sh * 8), out(dw * dh * 8, 0);
    FILE* f = fopen(argv[7], "rb");
    if (!f || fread(in.data(), 1, in.size(), f) != in.size()) return 3;
    fclose(f);
    const Image src{sw, sh, DXGI_FORMAT_R16G16B16A16_FLOAT, sw * 8, in.data()}, dst{dw, dh, DXGI_FORMAT_R16G16B16A16_FLOAT, dw * 8, out.data()};
    HRESULT hr = E_INVALIDARG;
    if (!strcmp(argv[1], "point")) hr = _ResizePointFilter(src, dst);
    else if (!strcmp(argv[1], "box")) hr = _ResizeBoxFilter(src, filter, dst);
    else if (!strcmp(argv[1], "linear")) hr = _ResizeLinearFilter(src, filter, dst);
    else if (!strcmp(argv[1], "cubic")) hr = _ResizeCubicFilter(src, filter, dst);
    else if (!strcmp(argv[1], "triangle")) hr = _ResizeTriangleFilter(src, filter, dst);
    if (hr != S_OK) return 4;
    f = fopen(argv[8], "wb");
    fwrite(out.data(), 1, out.size(), f);
    fclose(f);
    return 0;
}
"""

LINEAR_TABLE = np.dtype([("u", "<i4", 2), ("w", "<f4", 2)])
CUBIC_TABLE = np.dtype([("u", "<i4", 4), ("x", "<f4")])
TRIANGLE_TABLE = np.dtype([("idx", "<i4", 2), ("w", "<f4")])
TABLE_DTYPES = {"linear": LINEAR_TABLE, "cubic": CUBIC_TABLE, "triangle": TRIANGLE_TABLE}


def build(ref_root, work):
    dxtex = os.path.join(ref_root, "3rdParty", "DirectXTex", "DirectXTex")
    with open(os.path.join(dxtex, "Filters.h"), encoding="latin-1") as f:
        fl = f.readlines()
    with open(os.path.join(dxtex, "DirectXTexResize.cpp"), encoding="latin-1") as f:
        rl = f.readlines()
    filters = MG.cut(fl, "g_boxScale =", "g_boxScale3D =") + MG.cut(fl, "#define AVERAGE4(", "#define AVERAGE8(") \
        + MG.cut(fl, "struct LinearFilter", "#define TRILINEAR_INTERPOLATE(") \
        + MG.cut(fl, "g_cubicThird =", "// Triangle filtering helpers") + MG.cut(fl, "namespace TriangleFilter", "}; // namespace") + ["}\n"]
    resize = MG.cut(rl, "static HRESULT _ResizePointFilter(", "//--- Custom filter resize ---")
    with open(os.path.join(work, "cut_filters.inc"), "w") as f:
        f.writelines(filters)
    with open(os.path.join(work, "cut_resize.inc"), "w") as f:
        f.writelines(resize)
    with open(os.path.join(work, "harness.cpp"), "w") as f:
        f.write(HARNESS)
    exe = os.path.join(work, "resize_ref")
    subprocess.run(["g++", "-std=c++17", "-O1", "-w", "-ffp-contract=off", "-I", os.path.join(ROOT, "oracle", "ref_build", "dxmath_stub"), "-I", work,
                    os.path.join(work, "harness.cpp"), "-o", exe], check=True)
    return exe


def run_level(exe, work, filt, addr, src, dw, dh):
    sh, sw = src.shape[:2]
    a, b = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
    np.ascontiguousarray(src).tofile(a)
    bits = 0x30 if addr == "mirror" else (1 if "u" in addr else 0) | (2 if "v" in addr else 0)       # TEX_FILTER_WRAP_U / _V, TEX_FILTER_MIRROR_U | _V
    subprocess.run([exe, filt, str(bits), str(sw), str(sh), str(dw), str(dh), a, b], check=True)
    return np.fromfile(b, dtype=np.uint16).reshape(dh, dw, 4)


def main():
    ref_root = sys.argv[1]
    work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="resize_ref_")
    os.makedirs(work, exist_ok=True)
    exe = build(ref_root, work)
    arrays, pins = {}, {"cases": {}, "tables": {}}
    for sizes, seed in R.CASES:
        w, h = sizes[0]
        base = MF.seeded_half_image(h, w, seed)
        if w * h <= SMALL:
            arrays["in_" + R.sizes_name(sizes)] = base
        for filt, addr in R.variants(sizes):
            levels = [base]
            for dw, dh in sizes[1:]:
                levels.append(run_level(exe, work, filt, addr, levels[-1], dw, dh))
            name = R.case_name(filt, addr, sizes)
            stored = [int(l.shape[0] * l.shape[1] <= SMALL) for l in levels[1:]]
            pins["cases"][name] = {"filter": filt, "address": addr, "sizes": [list(s) for s in sizes], "seed": seed, "stored": stored,
                                   "input_sha256": hashlib.sha256(base.tobytes()).hexdigest(),
                                   "levels_sha256": hashlib.sha256(b"".join(np.ascontiguousarray(l).tobytes() for l in levels[1:])).hexdigest()}
            for i, l in enumerate(levels[1:]):
                if stored[i]:
                    arrays[f"{name}_l{i + 1}"] = l
    uncovered = []
    for source, dest in R.table_pairs():
        for kind, address in R.TABLE_VARIANTS:
            if kind == "linear" and address == 1 and dest >= source and source > 1:
                continue
            dst = os.path.join(work, "table.bin")
            subprocess.run([exe, kind + "table", str(address), str(source), str(dest), dst], check=True)
            rec = np.fromfile(dst, dtype=TABLE_DTYPES[kind])
            name = R.table_name(kind, address, source, dest)
            pins["tables"][name] = {"entries": int(rec.size), "sha256": hashlib.sha256(rec.tobytes()).hexdigest()}
            if kind == "triangle":
                missing = sorted(set(range(dest)) - set(int(d) for d in rec["idx"][:, 1]))
                pins["tables"][name]["destinations_without_entry"] = len(missing)
                if missing:
                    uncovered.append((name, missing[:8]))
            arrays[name + "_i"] = rec["u" if kind != "triangle" else "idx"].copy()
            arrays[name + "_w"] = rec["w" if kind != "cubic" else "x"].copy()
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "resize_ref.npz"), **arrays)
    with open(os.path.join(gold, "resize_ref_sha256.json"), "w") as f:
        json.dump(pins, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(pins["cases"]), "cases,", len(pins["tables"]), "tables ->", gold, "|", os.path.getsize(os.path.join(gold, "resize_ref.npz")), "bytes")
    print("triangle tables that leave a destination without an entry:", uncovered or "none")


if __name__ == "__main__":
    main()
