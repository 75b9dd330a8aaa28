"""What the signed normal-map path costs, device-resident, per texel kind (int8 RGBA8_SNORM, half RGBA16F, float RGBA32F): a crop of a real
normal map (tests/golden/normals_crop_128.npy) recentred to signed values and tiled to size, and a synthetic noise-perturbed +Z field.  One
run: every leg of a content alternates call by call with the others, so that whatever the clocks do they do to all of them.  A call = the
entry point(s) on device pointers followed by a synchronise of the stream, inside a host clock (time.perf_counter).  Per leg: the median of
reps x inner calls (default 7 x 5 = 35), the fastest call, p10 and p90.

Legs (ops = flip X | flip Y | normalise unless said otherwise; K = int8, half, float):
  a            CompressBlocksBC5S of an int8 surface; a_bc5 / a_bc5n: CompressBlocksBC5 and itwCompressNormalMapBC5 of the same bytes, whose
               kernels share the file (and *_parent: the same three through --parent-lib=PATH, another build's libispc_texcomp.so, same run)
  b_K          itwQuantizeNormalMapChain into an int8 scratch, then CompressBlocksBC5S of the scratch
  c_K, c0_K    itwCompressNormalMapBC5S with ops 7 and ops 0 (c0_int8 is CompressBlocksBC5S itself)
  d_K          itwQuantizeNormalMapChain alone (also as a fraction of 8 TB/s: read of the source + write of the int8 image)
  e_K_mipped   a 1024^2 cube with mips through itwCompressSignedNormalMapMipped
  e_K_stages   the same chain from a ready RGBA16F mip chain: itwQuantizeNormalMapChain per level + itwCompressImageChainEx (the mip filter
               is not in this leg: it is the same launches either way)

One JSON object per content per line (stdout, and appended to profiles/normal_snorm_timing.jsonl unless --no-save).
Usage: python tools/normal_snorm_timing.py [reps] [inner] [--size=N] [--parent-lib=PATH] [--label=TEXT] [--no-save] [--out=PATH]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
import numpy as np                      # noqa: E402
import itw_amd                          # noqa: E402

OPS = 7
PEAK_BYTES_PER_US = 8.0e6               # 8 TB/s
KINDS = (("int8", 4), ("half", 8), ("float", 16))


def opt(name, default):
    return next((a[len(name) + 3:] for a in sys.argv if a.startswith("--" + name + "=")), default)


def contents(size):
    """float32 (size, size, 4) signed vectors, not unit length: the normalise has work to do"""
    crop = np.load(os.path.join(ROOT, "tests", "golden", "normals_crop_128.npy"))
    reps = (size + crop.shape[0] - 1) // crop.shape[0]
    tiled = np.tile(crop, (reps, reps, 1))[:size, :size]
    tiled = ((tiled.astype(np.float32) - np.float32(128.0)) * np.float32(1.0 / 127.0)).astype(np.float32)
    rng = np.random.default_rng(1)
    synth = np.ones((size, size, 4), np.float32)
    synth[..., :2] = rng.normal(0.0, 0.25, (size, size, 2)) * 0.8
    synth[..., 2] = 0.8
    return {"normals_crop_tiled": tiled, "synthetic_plus_z": synth}


def as_kind(v, kind):
    if kind == "int8":
        return np.clip(np.rint(v * 127.0), -127, 127).astype(np.int8)
    return v.astype(np.float16).view(np.int16) if kind == "half" else np.ascontiguousarray(v, dtype=np.float32)


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    inner = int(args[1]) if len(args) > 1 else 5
    size = int(opt("size", 4096))
    out_path = opt("out", os.path.join(ROOT, "profiles", "normal_snorm_timing.jsonl"))
    L = itw_amd.lib()
    S = itw_amd.RgbaSurface
    parent = None
    if opt("parent-lib", None):
        parent = C.CDLL(opt("parent-lib", None), mode=C.RTLD_LOCAL)
        parent.itwSetStream.argtypes = [C.c_void_p]
        parent.itwSetStream.restype = None
        for name in ("CompressBlocksBC5S", "CompressBlocksBC5"):
            getattr(parent, name).argtypes = [C.POINTER(S), C.c_void_p]
            getattr(parent, name).restype = None
        parent.itwCompressNormalMapBC5.argtypes = [C.POINTER(S), C.c_void_p, C.c_uint32]
        parent.itwCompressNormalMapBC5.restype = None
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    for lib in (L, parent):
        if lib is not None:
            lib.itwSetStream(stream.cuda_stream)
            lib.itwWarmupBC45()
            lib.itwWarmupBC45S()

    for cname, v in contents(size).items():
        src = {k: torch.from_numpy(as_kind(v, k)).to(dev) for k, _ in KINDS}
        surf = {k: S(src[k].data_ptr(), size, size, size * tb) for k, tb in KINDS}
        scratch = torch.empty((size, size, 4), dtype=torch.int8, device=dev)
        s_scr = S(scratch.data_ptr(), size, size, size * 4)
        out = torch.empty((size // 4) ** 2 * 16, dtype=torch.uint8, device=dev)
        legs = [("a", lambda: L.CompressBlocksBC5S(C.byref(surf["int8"]), out.data_ptr())),
                ("a_bc5", lambda: L.CompressBlocksBC5(C.byref(surf["int8"]), out.data_ptr())),
                ("a_bc5n", lambda: L.itwCompressNormalMapBC5(C.byref(surf["int8"]), out.data_ptr(), OPS))]
        if parent:
            legs += [("a_parent", lambda: parent.CompressBlocksBC5S(C.byref(surf["int8"]), out.data_ptr())),
                     ("a_bc5_parent", lambda: parent.CompressBlocksBC5(C.byref(surf["int8"]), out.data_ptr())),
                     ("a_bc5n_parent", lambda: parent.itwCompressNormalMapBC5(C.byref(surf["int8"]), out.data_ptr(), OPS))]
        keep = []                                                 # what the lambdas' pointers point into

        def quant_then_encode(s, tb):
            L.itwQuantizeNormalMapChain(C.byref(s), tb, C.byref(s_scr), 1, OPS)
            L.CompressBlocksBC5S(C.byref(s_scr), out.data_ptr())

        for k, tb in KINDS:
            s = surf[k]
            legs += [(f"b_{k}", lambda s=s, tb=tb: quant_then_encode(s, tb)),
                     (f"c_{k}", lambda s=s, tb=tb: L.itwCompressNormalMapBC5S(C.byref(s), tb, out.data_ptr(), OPS)),
                     (f"c0_{k}", lambda s=s, tb=tb: L.itwCompressNormalMapBC5S(C.byref(s), tb, out.data_ptr(), 0)),
                     (f"d_{k}", lambda s=s, tb=tb: L.itwQuantizeNormalMapChain(C.byref(s), tb, C.byref(s_scr), 1, OPS))]
        if size >= 3072:                                          # leg e: six 1024^2 faces cut from the content
            for k, tb in KINDS:
                bases = [src[k][(f // 3) * 1024:(f // 3) * 1024 + 1024, (f % 3) * 1024:(f % 3) * 1024 + 1024].contiguous() for f in range(6)]
                arr_b = itw_amd.abi._surfaces(bases)
                half_bases = [torch.from_numpy(as_kind(v[(f // 3) * 1024:(f // 3) * 1024 + 1024, (f % 3) * 1024:(f % 3) * 1024 + 1024], "half")).to(dev) for f in range(6)]
                levels = [lv for ch in itw_amd.generate_mips(half_bases) for lv in ch]
                q = [torch.empty(tuple(lv.shape), dtype=torch.int8, device=dev) for lv in levels]
                arr_l, arr_q = itw_amd.abi._surfaces(levels), itw_amd.abi._surfaces(q)
                chain_out = torch.empty(itw_amd.chain_bytes("bc5_snorm", q), dtype=torch.uint8, device=dev)
                keep += [bases, levels, q, arr_b, arr_l, arr_q, chain_out]

                def stages(arr_l=arr_l, arr_q=arr_q, n=len(levels), chain_out=chain_out):
                    L.itwQuantizeNormalMapChain(C.cast(arr_l, C.c_void_p), 8, C.cast(arr_q, C.c_void_p), n, 4)
                    L.itwCompressImageChainEx(C.cast(arr_q, C.c_void_p), n, chain_out.data_ptr(), 84, None, None, None)

                legs += [(f"e_{k}_mipped", lambda arr_b=arr_b, tb=tb, chain_out=chain_out:
                          L.itwCompressSignedNormalMapMipped(C.cast(arr_b, C.c_void_p), 6, 0, tb, OPS, chain_out.data_ptr(), 84, None, None))]
                if k == "half":
                    legs.append(("e_half_stages", stages))

        for _ in range(3):                                        # warm-up: code objects, tables, the thread's buffers, clocks
            for _, call in legs:
                call()
        stream.synchronize()
        times = {name: [] for name, _ in legs}
        for _ in range(reps):
            for _ in range(inner):
                for name, call in legs:                           # the legs alternate
                    t0 = time.perf_counter()
                    call()
                    stream.synchronize()
                    times[name].append((time.perf_counter() - t0) * 1e6)
        row = {"content": cname, "size": size, "ops": OPS, "reps": reps, "inner": inner, "calls_per_leg": reps * inner, "label": opt("label", ""),
               "parent_lib": bool(parent), "device": itw_amd.device_info(), "unit": "us per call, host clock around call(s) + stream synchronise"}
        for name, t in times.items():
            t = np.sort(np.array(t))
            row[name] = {"median_us": round(float(np.median(t)), 2), "min_us": round(float(t[0]), 2),
                         "p10_us": round(float(np.percentile(t, 10)), 2), "p90_us": round(float(np.percentile(t, 90)), 2)}
        med = lambda k: row[k]["median_us"]
        for k, tb in KINDS:
            row[f"c_over_b_{k}"] = round(med(f"c_{k}") / med(f"b_{k}"), 3)
            row[f"c_over_a_{k}"] = round(med(f"c_{k}") / med("a"), 3)
            row[f"d_{k}_fraction_of_8TBs"] = round(size * size * (tb + 4) / med(f"d_{k}") / PEAK_BYTES_PER_US, 3)
        print(json.dumps(row), flush=True)
        if "--no-save" not in sys.argv:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "a") as f:
                f.write(json.dumps(row) + "\n")
        del keep


if __name__ == "__main__":
    main()
