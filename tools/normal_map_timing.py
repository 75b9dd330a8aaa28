"""What the normal-map stages cost, device-resident, on tangent-space normal maps: a crop of a real normal map (tests/golden/normals_crop_128.npy)
tiled to size, and a synthetic noise-perturbed +Z field.  One run: every leg of a content alternates call by call with the others, so that
whatever the clocks do they do to all of them.  A call = the entry point(s) on device pointers followed by a synchronise of the stream, inside
a host clock (time.perf_counter).  Per leg: the median of reps x inner calls (default 7 x 5 = 35), the fastest call, p10 and p90.

Legs (ops = flip X | flip Y | normalise unless said otherwise):
  a        CompressBlocksBC5 alone (and a_parent: the same through --parent-lib=PATH, another build's libispc_texcomp.so, in the same run)
  b        itwPrepareNormalMapChain in place on a scratch copy, then CompressBlocksBC5 (the copy is restored outside the clock)
  b_copy   the same with the scratch copy counted: hipMemcpyAsync device to device first -- what a caller who keeps the source pays
  c        itwCompressNormalMapBC5
  d8, d16  itwPrepareNormalMapChain alone, RGBA8 and RGBA16F (also as a fraction of 8 TB/s: read + write of the surface)
  e_*      a 1024^2 cube map with mips (66 images), BC5 and BC7 `basic`: itwCompressNormalMapChain against itwPrepareNormalMapChain in place
           (restored outside the clock) + itwCompressImageChainEx
  f_ops4, f_ops0   size^2 BC5 through the chain call with normalise against without: the price of giving up the in-place route

One JSON object per content per line (stdout, and appended to profiles/normal_map_timing.jsonl unless --no-save).
Usage: python tools/normal_map_timing.py [reps] [inner] [--size=N] [--parent-lib=PATH] [--label=TEXT] [--no-save] [--out=PATH]"""
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


def opt(name, default):
    return next((a[len(name) + 3:] for a in sys.argv if a.startswith("--" + name + "=")), default)


def contents(size):
    crop = np.load(os.path.join(ROOT, "tests", "golden", "normals_crop_128.npy"))
    reps = (size + crop.shape[0] - 1) // crop.shape[0]
    tiled = np.ascontiguousarray(np.tile(crop, (reps, reps, 1))[:size, :size])
    rng = np.random.default_rng(1)
    n = np.empty((size, size, 3), np.float32)
    n[..., :2] = rng.normal(0.0, 0.25, (size, size, 2))
    n[..., 2] = 1.0
    synth = np.full((size, size, 4), 255, np.uint8)
    synth[..., :3] = np.clip(n * 100.0 + 128.0, 0, 255).astype(np.uint8)       # not unit length: the normalise has work to do
    return {"normals_crop_tiled": tiled, "synthetic_plus_z": synth}


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    inner = int(args[1]) if len(args) > 1 else 5
    size = int(opt("size", 4096))
    out_path = opt("out", os.path.join(ROOT, "profiles", "normal_map_timing.jsonl"))
    L = itw_amd.lib()
    parent = None
    if opt("parent-lib", None):
        parent = C.CDLL(opt("parent-lib", None), mode=C.RTLD_LOCAL)
        parent.itwSetStream.argtypes = [C.c_void_p]
        parent.itwSetStream.restype = None
        parent.CompressBlocksBC5.argtypes = [C.POINTER(itw_amd.RgbaSurface), C.c_void_p]
        parent.CompressBlocksBC5.restype = None
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    L.itwSetStream(stream.cuda_stream)
    if parent:
        parent.itwSetStream(stream.cuda_stream)
        parent.itwWarmupBC45()
    L.itwWarmupBC45()
    S = itw_amd.RgbaSurface
    s7 = itw_amd.bc7_profile("basic")

    for cname, img in contents(size).items():
        src = torch.from_numpy(img).to(dev)
        scratch = src.clone()
        half = torch.from_numpy(((img.astype(np.float32) - 128.0) / 100.0).astype(np.float16).view(np.int16)).to(dev)
        out = torch.empty((size // 4) ** 2 * 16, dtype=torch.uint8, device=dev)
        s_src, s_scr = S(src.data_ptr(), size, size, size * 4), S(scratch.data_ptr(), size, size, size * 4)
        s_half = S(half.data_ptr(), size, size, size * 8)
        nbytes = size * size * 4
        # the chain of leg e: a 1024^2 cube with mips, faces cut from the content
        faces = [itw_amd.mip_chain(np.ascontiguousarray(img[(f // 3) * 1024:(f // 3) * 1024 + 1024, (f % 3) * 1024:(f % 3) * 1024 + 1024])) for f in range(6)] if size >= 3072 else []
        levels = [torch.from_numpy(lv).to(dev) for face in faces for lv in face]
        lv_scr = [t.clone() for t in levels]
        arr_src, arr_scr = itw_amd.abi._surfaces(levels), itw_amd.abi._surfaces(lv_scr)
        chain_out = torch.empty(max(16, itw_amd.chain_bytes("bc7", levels) if levels else 16), dtype=torch.uint8, device=dev)
        one_src = itw_amd.abi._surfaces([src])
        p7 = C.cast(C.byref(s7), C.c_void_p)

        def restore():
            scratch.copy_(src)

        def restore_chain():
            for a, b in zip(lv_scr, levels):
                a.copy_(b)

        def leg_b():
            L.itwPrepareNormalMapChain(C.byref(s_scr), 1, 4, OPS)
            L.CompressBlocksBC5(C.byref(s_scr), out.data_ptr())

        def leg_b_copy():
            hip.hipMemcpyAsync(scratch.data_ptr(), src.data_ptr(), nbytes, 3, stream.cuda_stream)
            leg_b()

        def chain_two_calls(fmt, sp):
            L.itwPrepareNormalMapChain(C.cast(arr_scr, C.c_void_p), len(levels), 4, OPS)
            L.itwCompressImageChainEx(C.cast(arr_scr, C.c_void_p), len(levels), chain_out.data_ptr(), fmt, sp, None, None)

        legs = [("a", None, lambda: L.CompressBlocksBC5(C.byref(s_src), out.data_ptr()))]
        if parent:
            legs.append(("a_parent", None, lambda: parent.CompressBlocksBC5(C.byref(s_src), out.data_ptr())))
        legs += [("b", restore, leg_b), ("b_copy", None, leg_b_copy),
                 ("c", None, lambda: L.itwCompressNormalMapBC5(C.byref(s_src), out.data_ptr(), OPS)),
                 ("d8", None, lambda: L.itwPrepareNormalMapChain(C.byref(s_scr), 1, 4, OPS)),
                 ("d16", None, lambda: L.itwPrepareNormalMapChain(C.byref(s_half), 1, 8, OPS))]
        if levels:
            legs += [("e_bc5_fused", None, lambda: L.itwCompressNormalMapChain(C.cast(arr_src, C.c_void_p), len(levels), chain_out.data_ptr(), 83, None, OPS, None, None)),
                     ("e_bc5_two_calls", restore_chain, lambda: chain_two_calls(83, None)),
                     ("e_bc7_basic_fused", None, lambda: L.itwCompressNormalMapChain(C.cast(arr_src, C.c_void_p), len(levels), chain_out.data_ptr(), 98, p7, OPS, None, None)),
                     ("e_bc7_basic_two_calls", restore_chain, lambda: chain_two_calls(98, p7))]
        legs += [("f_ops4", None, lambda: L.itwCompressNormalMapChain(C.cast(one_src, C.c_void_p), 1, out.data_ptr(), 83, None, 4, None, None)),
                 ("f_ops0", None, lambda: L.itwCompressNormalMapChain(C.cast(one_src, C.c_void_p), 1, out.data_ptr(), 83, None, 0, None, None))]

        for _ in range(3):                                        # warm-up: code objects, tables, the thread's buffers, clocks
            for _, before, call in legs:
                if before:
                    before()
                call()
        stream.synchronize()
        times = {name: [] for name, *_ in legs}
        for _ in range(reps):
            for _ in range(inner):
                for name, before, call in legs:                   # the legs alternate
                    if before:
                        before()
                        stream.synchronize()
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
        row["c_over_a"] = round(med("c") / med("a"), 3)
        row["c_over_b"] = round(med("c") / med("b"), 3)
        row["c_over_b_copy"] = round(med("c") / med("b_copy"), 3)
        row["d8_fraction_of_8TBs"] = round(2 * nbytes / med("d8") / PEAK_BYTES_PER_US, 3)
        row["d16_fraction_of_8TBs"] = round(4 * nbytes / med("d16") / PEAK_BYTES_PER_US, 3)
        print(json.dumps(row), flush=True)
        if "--no-save" not in sys.argv:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "a") as f:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
