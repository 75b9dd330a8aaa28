"""What encoding to an error budget costs (itwCompressImageRefined) against the calls it is made of, 4096^2, everything device-resident.

Surfaces: the bench surface (surfaces.ldr_smooth / hdr_smooth, bench.py's seeds) and the reference's baboon.png (tests/golden/inputs.npz)
tiled to the same size -- for BC6H its RGB as v / 255 in half floats, alpha 1.0.  Tier pairs: BC7 veryfast -> slow, BC6H fast -> slow.
Per surface and pair, in ONE run, the variants alternating within each repetition:
    first         CompressBlocks* with the first preset alone          (unchanged entry points: the baseline)
    refine        CompressBlocks* with the refine preset alone         (likewise)
    measure       itwMeasureBlocks of the first preset's stream
    refined_none  itwCompressImageRefined, max_block_sse = UINT64_MAX  (nothing listed)
    refined_10 / _30 / _100   ... at the budgets that list 10 %, 30 % and every block; the budgets come from a first call's error map
The refined call is synchronous, so EVERY variant is timed the same way: a host clock around `inner` calls, each followed by a stream
synchronise; after a warm-up of every variant; best, median and spread of `reps` repetitions.  Each refined row carries listed / replaced
and what the stream it wrote costs against the source (itwMeasureBlocks: sum of squared code differences, and itwStatsPsnr for BC7).
Derived: fixed_overhead_ms = refined_none - first - measure; excess_at_100_ms = refined_100 - first - refine (medians).
One JSON object per line (stdout, and appended to profiles/refine_timing.jsonl unless --no-save).

--target: what letting the device pick the budget costs (itwCompressImageRefinedTo), same surfaces, pairs and timing method, appended to
profiles/refine_target_timing.jsonl.  At 10 % and 30 % of the blocks, alternating in one run:
    known_P   itwCompressImageRefined with the budget already known (the T the new call reports for the same rank): the floor
    to_P      itwCompressImageRefinedTo, max_listed = P % of the blocks; to_P - known_P is the select's cost
    route_P   what a caller had to do before: a nothing-listed call that fills a device block map, the map's download, np.partition for
              the (k+1)-th largest, and the second call -- which repeats the first tier
and policy B at two targets a third and two thirds of the way from the first preset's to the refine preset's quality (BC7: in dB through
itwPsnrToTotalSse; BC6H: in summed error): rounds, blocks listed, what was reached, ms.
Usage: python tools/refine_timing.py [reps] [inner] [--target] [--no-save] [--out=PATH] [--size=N]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
import numpy as np                      # noqa: E402
import itw_amd                          # noqa: E402
from itw_amd import surfaces           # noqa: E402

PAIRS = [("bc7", "veryfast", "slow"), ("bc6h", "fast", "slow")]
U64_MAX = 2 ** 64 - 1


def _surface(name, fmt, size):
    if name == "bench":
        return surfaces.hdr_smooth(size, size, seed=surfaces.SEED + 3) if fmt == "bc6h" else surfaces.ldr_smooth(size, size, seed=surfaces.SEED)
    z = np.load(os.path.join(ROOT, "tests", "golden", "inputs.npz"))["baboon"]
    reps = -(-size // z.shape[0])
    img = np.ascontiguousarray(np.tile(z, (reps, reps, 1))[:size, :size])
    if fmt == "bc6h":
        img = (img.astype(np.float32) / 255.0).astype(np.float16).view(np.uint16)
        img[..., 3] = 0x3C00
    return img


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    inner = int(args[1]) if len(args) > 1 else 5
    save = "--no-save" not in sys.argv
    size = int(next((a[7:] for a in sys.argv if a.startswith("--size=")), 4096))
    out_path = next((a[6:] for a in sys.argv if a.startswith("--out=")), os.path.join(ROOT, "profiles", "refine_timing.jsonl"))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L = itw_amd.lib()
    L.itwSetStream(torch.cuda.current_stream(dev).cuda_stream)
    nb = (size // 4) ** 2
    rows = []
    for content in ("bench", "baboon_tiled"):
        for fmt, first, refine in PAIRS:
            host = _surface(content, fmt, size)
            img = torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host).to(dev)
            profile = itw_amd.bc7_profile if fmt == "bc7" else itw_amd.bc6h_profile
            s1, s2 = profile(first), profile(refine)
            surf = itw_amd.RgbaSurface(img.data_ptr(), size, size, img.stride(0) * img.element_size())
            out = torch.empty(nb * 16, dtype=torch.uint8, device=dev)
            first_stream = torch.empty(nb * 16, dtype=torch.uint8, device=dev)
            raw = torch.zeros(C.sizeof(itw_amd.ErrorStats), dtype=torch.uint8, device=dev)
            st = itw_amd.RefineStats()

            def refined(budget, bmap=None):
                ok = L.itwCompressImageRefined(C.byref(surf), out.data_ptr(), itw_amd.DXGI_FORMAT[fmt], C.addressof(s1), C.addressof(s2), 7, budget,
                                               C.addressof(st), C.sizeof(st), bmap.data_ptr() if bmap is not None else None, None)
                assert ok, itw_amd.last_error()

            # the budgets, from a first call's map
            bmap = torch.empty(nb, dtype=torch.int64, device=dev)
            refined(U64_MAX, bmap)
            s = np.sort(bmap.cpu().numpy())
            budgets = {"refined_none": U64_MAX, "refined_10": int(s[nb - nb // 10 - 1]), "refined_30": int(s[nb - (3 * nb) // 10 - 1]), "refined_100": 0}
            itw_amd.compress(fmt, img, s1, out=first_stream)
            torch.cuda.synchronize()

            variants = {"first": lambda: itw_amd.compress(fmt, img, s1, out=out), "refine": lambda: itw_amd.compress(fmt, img, s2, out=out),
                        "measure": lambda: itw_amd.measure_async(fmt, first_stream, img, raw)}
            for name, budget in budgets.items():
                variants[name] = (lambda b: lambda: refined(b))(budget)

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                    torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3 / inner

            for fn in variants.values():                         # warm-up: code objects, workspaces, the refined call's scratch at its largest
                fn(); fn()
            torch.cuda.synchronize()
            times = {name: [] for name in variants}
            for _ in range(reps):
                for name, fn in variants.items():
                    times[name].append(timed(fn))
            row = {"content": content, "format": fmt, "first": first, "refine": refine, "size": size, "blocks": nb, "reps": reps, "inner": inner,
                   "timing": "host clock around calls that each end in a stream synchronise", "device": itw_amd.device_info(), "variants": {}}
            for name, fn in variants.items():
                t = sorted(times[name])
                v = {"ms": round(t[0], 4), "median_ms": round(t[len(t) // 2], 4), "spread": round((t[-1] - t[0]) / t[0], 3)}
                if name != "measure":                            # what the stream this variant writes costs against the source
                    fn()
                    if name.startswith("refined"):
                        v.update(budget=budgets[name], listed=int(st.listed), replaced=int(st.replaced), sse_first=int(st.sse_first), sse_final=int(st.sse_final))
                    es = itw_amd.measure(fmt, out, img)
                    v["sse_rgb"] = sum(int(es.sse[c]) for c in range(3))
                    if fmt == "bc7":
                        v["psnr_rgb_db"] = round(es.psnr("rgb"), 4)
                row["variants"][name] = v
            med = {name: row["variants"][name]["median_ms"] for name in variants}
            row["fixed_overhead_ms"] = round(med["refined_none"] - med["first"] - med["measure"], 4)
            row["excess_at_100_ms"] = round(med["refined_100"] - med["first"] - med["refine"], 4)
            row["refined_30_vs_refine"] = round(med["refined_30"] / med["refine"], 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
    if save and rows:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def main_target():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    inner = int(args[1]) if len(args) > 1 else 5
    save = "--no-save" not in sys.argv
    size = int(next((a[7:] for a in sys.argv if a.startswith("--size=")), 4096))
    out_path = next((a[6:] for a in sys.argv if a.startswith("--out=")), os.path.join(ROOT, "profiles", "refine_target_timing.jsonl"))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L = itw_amd.lib()
    L.itwSetStream(torch.cuda.current_stream(dev).cuda_stream)
    nb = (size // 4) ** 2
    rows = []
    for content in ("bench", "baboon_tiled"):
        for fmt, first, refine in PAIRS:
            host = _surface(content, fmt, size)
            img = torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host).to(dev)
            profile = itw_amd.bc7_profile if fmt == "bc7" else itw_amd.bc6h_profile
            s1, s2 = profile(first), profile(refine)
            surf = itw_amd.RgbaSurface(img.data_ptr(), size, size, img.stride(0) * img.element_size())
            out = torch.empty(nb * 16, dtype=torch.uint8, device=dev)
            bmap = torch.empty(nb, dtype=torch.int64, device=dev)
            st, ts = itw_amd.RefineStats(), itw_amd.RefineTargetStats()

            def known(budget, bm=None):
                ok = L.itwCompressImageRefined(C.byref(surf), out.data_ptr(), itw_amd.DXGI_FORMAT[fmt], C.addressof(s1), C.addressof(s2), 7, budget,
                                               C.addressof(st), C.sizeof(st), bm.data_ptr() if bm is not None else None, None)
                assert ok, itw_amd.last_error()

            def to(max_listed, target=U64_MAX):
                pol = itw_amd.RefinePolicy(max_listed, target)
                ok = L.itwCompressImageRefinedTo(C.byref(surf), out.data_ptr(), itw_amd.DXGI_FORMAT[fmt], C.addressof(s1), C.addressof(s2), 7,
                                                 C.addressof(pol), C.sizeof(pol), C.addressof(ts), C.sizeof(ts), None, None)
                assert ok, itw_amd.last_error()

            def route(k):
                known(U64_MAX, bmap)
                e = bmap.cpu().numpy()
                known(int(np.partition(e, nb - 1 - k)[nb - 1 - k]))      # the (k + 1)-th largest

            ranks = {"10": nb // 10, "30": (3 * nb) // 10}
            variants, info = {}, {}
            for p, k in ranks.items():
                to(k)
                t = int(ts.budget[0])
                info[p] = {"max_listed": k, "budget": t, "listed": int(ts.total.listed), "replaced": int(ts.total.replaced), "sse_final": int(ts.total.sse_final)}
                known(t)
                assert (int(st.listed), int(st.sse_final)) == (info[p]["listed"], info[p]["sse_final"])
                route(k)
                assert (int(st.listed), int(st.sse_final)) == (info[p]["listed"], info[p]["sse_final"])
                variants["known_" + p] = (lambda b: lambda: known(b))(t)
                variants["to_" + p] = (lambda n: lambda: to(n))(k)
                variants["route_" + p] = (lambda n: lambda: route(n))(k)
            # policy B: targets between the two presets
            known(0)
            sse_lo, sse_hi = int(st.sse_final), int(st.sse_first)       # every block refined; the first tier alone
            targets = {}
            for name, f in (("third", 1.0 / 3.0), ("two_thirds", 2.0 / 3.0)):
                if fmt == "bc7":
                    db = [10.0 * np.log10(255.0 ** 2 * size * size * 3 / float(v)) for v in (sse_hi, sse_lo)]
                    want_db = db[0] + f * (db[1] - db[0])
                    targets[name] = {"target_psnr_db": round(want_db, 4), "target_sse": itw_amd.psnr_to_total_sse(fmt, size, size, want_db)}
                else:
                    targets[name] = {"target_sse": int(sse_hi - f * (sse_hi - sse_lo))}
                variants["target_" + name] = (lambda v: lambda: to(U64_MAX, v))(targets[name]["target_sse"])

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                    torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3 / inner

            for fn in variants.values():
                fn(); fn()
            torch.cuda.synchronize()
            times = {name: [] for name in variants}
            for _ in range(reps):
                for name, fn in variants.items():
                    times[name].append(timed(fn))
            row = {"content": content, "format": fmt, "first": first, "refine": refine, "size": size, "blocks": nb, "reps": reps, "inner": inner,
                   "timing": "host clock around calls that each end in a stream synchronise", "device": itw_amd.device_info(),
                   "sse_first": sse_hi, "sse_all_refined": sse_lo, "variants": {}}
            for name, fn in variants.items():
                t = sorted(times[name])
                v = {"ms": round(t[0], 4), "median_ms": round(t[len(t) // 2], 4), "spread": round((t[-1] - t[0]) / t[0], 3)}
                if name.startswith("target_"):
                    fn()
                    v.update(targets[name[7:]], rounds=int(ts.rounds), target_met=int(ts.target_met), listed=int(ts.total.listed),
                             listed_per_round=[int(x) for x in ts.listed], replaced=int(ts.total.replaced), sse_final=int(ts.total.sse_final))
                    if fmt == "bc7":
                        v["psnr_rgb_db"] = round(10.0 * np.log10(255.0 ** 2 * size * size * 3 / float(ts.total.sse_final)), 4)
                else:
                    v.update(info[name.split("_")[1]])
                row["variants"][name] = v
            med = {name: row["variants"][name]["median_ms"] for name in variants}
            for p in ranks:
                row["select_cost_ms_" + p] = round(med["to_" + p] - med["known_" + p], 4)
                row["to_vs_route_" + p] = round(med["to_" + p] / med["route_" + p], 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
    if save and rows:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main_target() if "--target" in sys.argv else main()
