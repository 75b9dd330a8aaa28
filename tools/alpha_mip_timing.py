"""What the mip rules for cut-out textures cost (itwGenerateMipChainAlpha; include/itw_dispatch.h "Mip chains of cut-out textures"), in the
method of tools/mipgen_timing.py: device-resident chains, a call = the entry point followed by a synchronise of the stream, inside a host
clock (time.perf_counter); the legs of a row alternate call by call in one run; per leg the median of reps x inner calls (default 7 x 5 =
35), the fastest call, p10 and p90 -- the run's own spread.

Rows (one JSON object per line; stdout, and appended to profiles/alpha_mip_timing.jsonl unless --no-save): a 4096^2 RGBA8 chain and a
1024^2 cube, each on cut-out content (alpha spiked at 0 and 255, soft edges) and on uniform-noise alpha.  Legs:
  plain, weight, coverage, both          itwGenerateMipChainAlpha with neither, one or both rules on the default (pyramid) route; r = 128
  *_per_level                            the same with ITW_MIP_PER_LEVEL
  plain_parent, plain_parent_per_level   itwGenerateMipChain of another build of the library (--lib=PATH, the parent commit's), same job
  coverage_hist_spikes / _hist_lds       `coverage` through the hooks build with either histogram kernel (itwTestAlphaHistVariant 1 / 0)
  coverage_beside_caller, caller_today   a pair of its own, alternating: `coverage` again, and what a caller does without the rule: itwGenerateMipChain, every level downloaded, np.bincount and the
                                         table on the host, the new alpha uploaded
Usage: python tools/alpha_mip_timing.py [reps] [inner] [--lib=PATH] [--label=TEXT] [--no-save] [--out=PATH] [--only=SUBSTRING]
       python tools/alpha_mip_timing.py --trace      one call of plain, weight, coverage and both on the cube, for a kernel trace's launch counts"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                      # noqa: E402
import itw_amd                          # noqa: E402
import _alpha_mips as A                 # noqa: E402  (the contents of the tests)
from mipgen_timing import measure, opt  # noqa: E402

REF = 128


def host_coverage(torch, chains, ref):
    """The rule on the host over a generated chain: the histogram of every level >= 1 and its table in numpy, the alpha plane up again."""
    t = np.arange(1, 256)
    for ch in chains:
        n0 = ch[0].shape[0] * ch[0].shape[1]
        cov0 = int((ch[0][..., 3] >= ref).sum().item())
        for lv in ch[1:]:
            a = lv[..., 3].cpu().numpy()
            ge = np.cumsum(np.bincount(a.reshape(-1), minlength=256)[::-1])[::-1]
            k = (cov0 * a.size + n0 // 2) // n0
            best = int(t[np.lexsort((t, np.abs(t - ref), np.abs(ge[1:] - k)))[0]])
            if best != ref:
                lut = np.minimum(255, np.arange(256) * ref // best).astype(np.uint8)
                lv[..., 3].copy_(torch.from_numpy(lut[a]))


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    inner = int(args[1]) if len(args) > 1 else 5
    only = opt("only", "")
    trace = "--trace" in sys.argv
    out_path = opt("out", os.path.join(ROOT, "profiles", "alpha_mip_timing.jsonl"))
    L = itw_amd.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    L.itwSetStream(stream.cuda_stream)
    T = None if trace else itw_amd.test_lib()
    P = None
    if opt("lib", "") and not trace:
        P = C.CDLL(opt("lib", ""))
        P.itwGenerateMipChain.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32]
        P.itwGenerateMipChain.restype = C.c_int
        P.itwSetStream.argtypes = [C.c_void_p]
        P.itwSetStream(stream.cuda_stream)
    if T is not None:
        T.itwSetStream(stream.cuda_stream)

    def emit(row):
        row.update({"reps": reps, "inner": inner, "calls_per_leg": reps * inner, "label": opt("label", ""), "device": itw_amd.device_info(), "ref": REF,
                    "parent_lib": bool(P), "unit": "us per call, host clock around the call + stream synchronise"})
        print(json.dumps(row), flush=True)
        if "--no-save" not in sys.argv:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "a") as f:
                f.write(json.dumps(row) + "\n")

    tile = {"cutout": A.cutout(1024, 1024, 5, hole=False), "noise": A.noise(1024, 1024, 6)}
    for name, w, h, items in (("2d_4096", 4096, 4096, 1), ("cube_1024", 1024, 1024, 6)):
        for kind in ("cutout", "noise"):
            if only not in name + "_" + kind or (trace and (name, kind) != ("cube_1024", "cutout")):
                continue
            n = itw_amd.mip_levels(w, h)
            chains = []
            for i in range(items):
                base = torch.from_numpy(np.roll(np.tile(tile[kind], (h // 1024, w // 1024, 1)), 37 * i, axis=1)).to(dev)     # (the cut-out's period divides no tile)
                chains.append([base] + [torch.empty((max(1, h >> l), max(1, w >> l), 4), dtype=torch.uint8, device=dev) for l in range(1, n)])
            arr = C.cast(itw_amd.abi._surfaces([lv for ch in chains for lv in ch]), C.c_void_p)
            opts = {"plain": itw_amd.MipAlpha(0, 0), "weight": itw_amd.MipAlpha(1, 0), "coverage": itw_amd.MipAlpha(0, REF), "both": itw_amd.MipAlpha(1, REF)}
            ptr = {k: C.cast(C.byref(v), C.c_void_p) for k, v in opts.items()}

            def alpha_call(lib, which, flags):
                return lambda: lib.itwGenerateMipChainAlpha(arr, items, n, flags, ptr[which], None)

            if trace:
                for which in opts:
                    assert alpha_call(L, which, 0)() == 0
                stream.synchronize()
                return
            legs = []
            if P:
                legs.append(("plain_parent", lambda: P.itwGenerateMipChain(arr, items, n, 4, 0)))
                legs.append(("plain_parent_per_level", lambda: P.itwGenerateMipChain(arr, items, n, 4, 1)))
            for which in opts:
                legs.append((which, alpha_call(L, which, 0)))
                legs.append((which + "_per_level", alpha_call(L, which, itw_amd.MIP_PER_LEVEL)))
            def variant(spikes):
                call = alpha_call(T, "coverage", 0)
                return lambda: (T.itwTestAlphaHistVariant(spikes), call())

            legs.append(("coverage_hist_spikes", variant(1)))
            legs.append(("coverage_hist_lds", variant(0)))

            def today():
                L.itwGenerateMipChain(arr, items, n, 4, 0)
                host_coverage(torch, chains, REF)

            row = {"row": name + "_" + kind, "width": w, "height": h, "items": items, "levels": n}
            row.update(measure(legs, reps, inner, stream))
            # a pair of its own: its milliseconds on the host leave the device idle, which the leg behind it would pay for
            pair = measure([("coverage_beside_caller", alpha_call(L, "coverage", 0)), ("caller_today", today)], reps, inner, stream)
            row.update(pair)
            T.itwTestAlphaHistVariant(0)
            for leg in ("weight", "coverage", "both"):
                row[leg + "_over_plain"] = round(row[leg]["median_us"] / row["plain"]["median_us"], 3)
                row[leg + "_pyramid_over_per_level"] = round(row[leg]["median_us"] / row[leg + "_per_level"]["median_us"], 3)
            row["hist_spikes_over_hist_lds"] = round(row["coverage_hist_spikes"]["median_us"] / row["coverage_hist_lds"]["median_us"], 3)
            row["coverage_over_caller_today"] = round(row["coverage_beside_caller"]["median_us"] / row["caller_today"]["median_us"], 4)
            if P:
                row["plain_over_parent"] = round(row["plain"]["median_us"] / row["plain_parent"]["median_us"], 3)
            emit(row)
            del chains


if __name__ == "__main__":
    main()
