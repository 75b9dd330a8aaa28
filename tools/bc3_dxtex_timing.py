"""BC3 by DirectXTex's encoder (D3DXEncodeBC3, csrc/bc3_dxtex.hip) timed on the project's method, as tools/bc2_timing.py times BC2: a call =
the entry point followed by a synchronise of its stream, inside a host clock (time.perf_counter); the legs of a group alternate call by
call in one job; per leg the median of reps x inner calls (default 7 x 5 = 35), the fastest call and the p10-p90 spread over the median.
Run it twice (--label=run1 / run2): the difference between two runs is the noise floor of every comparison made here.

Groups (one JSON object per line on stdout, appended to profiles/bc3_dxtex_timing.jsonl unless --no-save):
  resident  4096^2 (--size=N), device-resident, through itwCompressImageSlicedEx with one slice: the new encoder plain, uniform, dither RGB,
            dither A, all flags; beside them, in the same build and job, BC2 plain (the same colour half, a 4-bit alpha half), BC1A plain
            (the colour half alone), the ISPC BC3 kernel and BC4 (DirectXTex's other OptimizeAlpha user).  Two contents: `cutout` (the
            BC1A / BC2 tools' content: most blocks fully transparent or fully opaque) and `bench` (bench.py's surface, smooth alpha: every
            block runs the Newton loop).  The new encoder's rows carry the ratios to the BC2, BC1A and ISPC BC3 medians of the same run,
            and `alpha_us`: its median minus BC1A's, what the alpha half and the 8 more bytes stored cost.
  sliced    the new encoder and BC2, plain, from pageable host memory in 64 slices with a progress callback.
  builds    --lib=PATH: another build's libispc_texcomp.so (the parent commit's) against this one on BC2, BC1A and ISPC BC3, resident.
  quality   itwMeasureBlocks' alpha SSE and largest alpha difference of three streams -- ISPC BC3, the new encoder plain and with
            ITW_BC_DITHER_A -- of a smooth alpha gradient and of bench.py's surface (1024^2 each).
Usage: python tools/bc3_dxtex_timing.py [reps] [inner] [--size=N] [--groups=resident,sliced,builds,quality] [--lib=PATH] [--label=TEXT] [--no-save]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np                      # noqa: E402
import itw_amd                          # noqa: E402
from itw_amd import surfaces            # noqa: E402
from bc1a_timing import alternate, cutout, opt, sliced_call      # noqa: E402


def gradient(size):
    """A smooth alpha gradient: alpha rises by one code every 16 texels along x with a slow wave in y (soft smoke, a UI shadow) over mid-grey noise."""
    y, x = np.mgrid[0:size, 0:size].astype(np.float32)
    img = np.empty((size, size, 4), dtype=np.uint8)
    img[..., :3] = np.random.default_rng(9).integers(96, 160, (size, size, 3), dtype=np.uint8)
    img[..., 3] = np.clip(np.rint(x / 16.0 + 24.0 * np.sin(y / 97.0) + 64.0), 0, 255).astype(np.uint8)
    return img


def main():
    import torch
    nums = [int(a) for a in sys.argv[1:] if a.isdigit()]
    reps, inner = nums[0] if nums else 7, nums[1] if len(nums) > 1 else 5
    size = int(opt("size", "4096"))
    groups = opt("groups", "resident,sliced,quality").split(",")
    label = opt("label", "")
    out_path = os.path.join(ROOT, "profiles", "bc3_dxtex_timing.jsonl")
    L = itw_amd.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.itwSetStream(torch.cuda.current_stream(dev).cuda_stream)
    sync = torch.cuda.synchronize
    mpix = size * size / 1e6
    rows = []

    def row(group, name, s, extra=None):
        r = {"tool": "bc3_dxtex_timing", "group": group, "leg": name, "size": size, "reps": reps * inner, "label": label, "device": itw_amd.device_info(), **s,
             "mpix_s": round(mpix / (s["median_us"] * 1e-6), 1)}
        r.update(extra or {})
        rows.append(r)
        print(json.dumps(r), flush=True)

    S = itw_amd.Bc1aSettings
    contents = {"cutout": lambda: cutout(size), "bench": lambda: surfaces.ldr_smooth(size, size, seed=surfaces.SEED)}
    if "resident" in groups:
        L.itwWarmupBC45()
        for cname, make in contents.items():
            d_img = torch.from_numpy(make()).to(dev)
            d_out = torch.empty(size * size, dtype=torch.uint8, device=dev)             # 16-byte blocks fit
            surf = itw_amd.RgbaSurface(d_img.data_ptr(), size, size, size * 4)
            spec = [("bc3_dxtex", "bc3_dxtex", S()), ("bc3_dxtex_uniform", "bc3_dxtex", S(uniform=True)), ("bc3_dxtex_dither_rgb", "bc3_dxtex", S(dither_rgb=True)),
                    ("bc3_dxtex_dither_a", "bc3_dxtex", S(dither_a=True)), ("bc3_dxtex_all_flags", "bc3_dxtex", S(0.5, True, True, True)),
                    ("bc2", "bc2", S()), ("bc1a", "bc1a", S()), ("bc3_ispc", "bc3", None), ("bc4", "bc4", None)]
            legs = [(name, sliced_call(L, fmt, st, surf, d_out.data_ptr(), size, 1 << 62, None)) for name, fmt, st in spec]
            res = alternate(legs, reps, inner, sync)
            for name, s in res.items():
                extra = {"content": cname}
                if name.startswith("bc3_dxtex"):
                    extra.update({"over_bc2": round(s["median_us"] / res["bc2"]["median_us"], 3), "over_bc1a": round(s["median_us"] / res["bc1a"]["median_us"], 3),
                                  "over_bc3_ispc": round(s["median_us"] / res["bc3_ispc"]["median_us"], 3),
                                  "alpha_us": round(s["median_us"] - res["bc1a"]["median_us"], 1)})
                row("resident", name, s, extra)
            del d_img, d_out
    if "sliced" in groups:
        img = cutout(size)
        out = np.empty(size * size, dtype=np.uint8)
        cb = itw_amd.PROGRESS_FUNC(lambda i, n, u: True)
        surf = itw_amd.RgbaSurface(img.ctypes.data, size, size, size * 4)
        st = S()
        legs = [(fmt, sliced_call(L, fmt, st, surf, out.ctypes.data, size, size * size // 64, C.cast(cb, C.c_void_p))) for fmt in ("bc3_dxtex", "bc2")]
        res = alternate(legs, reps, inner, sync)
        for name, s in res.items():
            row("sliced_host_64", name, s, {"content": "cutout", "over_bc2": round(s["median_us"] / res["bc2"]["median_us"], 3)})
    other = opt("lib", "")
    if "builds" in groups and other:
        # the other build is bound by hand: it lacks what this build's package binds
        P = C.CDLL(other, mode=os.RTLD_LOCAL)
        for lib in (P, L):
            lib.itwCompressImageSlicedEx.argtypes = [C.POINTER(itw_amd.RgbaSurface), C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
            lib.itwCompressImageSlicedEx.restype = C.c_bool
        P.itwSetStream.argtypes = [C.c_void_p]
        P.itwSetStream(torch.cuda.current_stream(dev).cuda_stream)
        d_img = torch.from_numpy(cutout(size)).to(dev)
        d_out = torch.empty(size * size, dtype=torch.uint8, device=dev)
        dsurf = itw_amd.RgbaSurface(d_img.data_ptr(), size, size, size * 4)
        legs = []
        kept = (("bc2", S()), ("bc1a", S()), ("bc3", None))          # (the calls hold pointers to the settings: they live as long as the legs)
        for fmt, st in kept:
            for build, lib in (("parent", P), ("this", L)):
                legs.append((f"{fmt}_resident_{build}", sliced_call(lib, fmt, st, dsurf, d_out.data_ptr(), size, 1 << 62, None)))
        res = alternate(legs, reps, inner, sync)
        for name, s in res.items():
            extra = {"content": "cutout"}
            if name.endswith("_this"):
                p = res[name[:-5] + "_parent"]
                extra.update({"over_parent": round(s["median_us"] / p["median_us"], 4),
                              "within_parent_spread": bool(abs(s["median_us"] - p["median_us"]) <= p["spread"] * p["median_us"])})
            row("builds", name, s, extra)
    if "quality" in groups:
        n = 1024
        for cname, img in (("alpha_gradient", gradient(n)), ("bench_surface", surfaces.ldr_smooth(n, n, seed=surfaces.SEED))):
            t = torch.from_numpy(img).to(dev)
            for name, fmt, st in (("bc3_ispc", "bc3", None), ("bc3_dxtex", "bc3_dxtex", S()), ("bc3_dxtex_dither_a", "bc3_dxtex", S(dither_a=True))):
                blocks = itw_amd.compress(fmt, t, st)
                sync()
                d = itw_amd.measure(fmt, blocks, t).as_dict()
                r = {"tool": "bc3_dxtex_timing", "group": "quality", "leg": name, "content": cname, "size": n, "label": label,
                     "alpha_sse": d["sse"][3], "alpha_max_abs": d["max_abs"][3], "rgb_sse": sum(d["sse"][:3]), "alpha_rmse": round((d["sse"][3] / (n * n)) ** 0.5, 4)}
                rows.append(r)
                print(json.dumps(r), flush=True)
    if "--no-save" not in sys.argv and rows:
        with open(out_path, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
