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

--chain: a whole mip chain or cube map to a budget in one call (itwCompressImageChainRefined) against the per-image pattern, same timing
method, appended to profiles/chain_refine_timing.jsonl.  The chains of tools/chain_timing.py: the 1024^2 BC7 cube map with mips (66
images) and the 2048^2 BC7 2D chain (12 images), veryfast -> slow, and the 512^2 BC6H cube map (60 images), fast -> slow; budgets that list
10 % and 30 % of the chain's blocks, from the first tier's map.  Legs, alternating in one run:
    per_image_P      per image: itwPadToMultipleOf4Device, then itwCompressImageRefined with that budget (the padding counts as error there)
    chain_P          one itwCompressImageChainRefined call; chain_stats_P: the same with image_stats
    chain_first / chain_refine   itwCompressImageChainEx with the first / the refine preset alone, for scale
    level0_single_P / level0_chain_P (the 2048^2 chain): itwCompressImageRefined of level 0 against a chain of that one image -- what the
                     packed copy and the scratch target cost
--label=TEXT adds "build": TEXT to every row (which build the lines came from).
Usage: python tools/refine_timing.py [reps] [inner] [--target | --chain] [--no-save] [--out=PATH] [--size=N] [--label=TEXT]"""
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
LABEL = next((a[8:] for a in sys.argv if a.startswith("--label=")), None)
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
            if LABEL:
                row["build"] = LABEL
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
            if LABEL:
                row["build"] = LABEL
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


# name, format, first, refine, top size (h, w), faces: the chains of tools/chain_timing.py
CHAINS = [("bc7_1024_cube", "bc7", "veryfast", "slow", (1024, 1024), 6),
          ("bc7_2048_2d", "bc7", "veryfast", "slow", (2048, 2048), 1),
          ("bc6h_512_cube", "bc6h", "fast", "slow", (512, 512), 6)]


def main_chain():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    inner = int(args[1]) if len(args) > 1 else 5
    save = "--no-save" not in sys.argv
    out_path = next((a[6:] for a in sys.argv if a.startswith("--out=")), os.path.join(ROOT, "profiles", "chain_refine_timing.jsonl"))
    label = next((a[8:] for a in sys.argv if a.startswith("--label=")), None)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L = itw_amd.lib()
    L.itwSetStream(torch.cuda.current_stream(dev).cuda_stream)
    rows = []
    for name, fmt, first, refine, (h, w), faces in CHAINS:
        gen = surfaces.hdr_smooth if fmt == "bc6h" else surfaces.ldr_smooth
        images = [lv for f in range(faces) for lv in itw_amd.mip_chain(gen(h, w, seed=100 + f))]
        px = 8 if fmt == "bc6h" else 4
        fcode = itw_amd.DXGI_FORMAT[fmt]
        profile = itw_amd.bc7_profile if fmt == "bc7" else itw_amd.bc6h_profile
        s1, s2 = profile(first), profile(refine)
        A, B = C.addressof(s1), C.addressof(s2)
        count = len(images)
        nblocks = [((lv.shape[0] + 3) // 4) * ((lv.shape[1] + 3) // 4) for lv in images]
        offs = [int(v) for v in np.cumsum([0] + nblocks)]
        nb = offs[-1]
        srcs = [torch.from_numpy(lv.view(np.int16) if lv.dtype == np.uint16 else lv).to(dev) for lv in images]
        surf_of = lambda t: itw_amd.RgbaSurface(t.data_ptr(), t.shape[1], t.shape[0], t.stride(0) * t.element_size())
        arr = (itw_amd.RgbaSurface * count)(*[surf_of(t) for t in srcs])
        ssurf = [surf_of(t) for t in srcs]
        padded = [torch.empty(((t.shape[0] + 3) // 4 * 4, (t.shape[1] + 3) // 4 * 4, 4), dtype=t.dtype, device=dev) for t in srcs]
        psurf = [surf_of(t) for t in padded]
        out = torch.empty(nb * 16, dtype=torch.uint8, device=dev)
        bmap = torch.empty(nb, dtype=torch.int64, device=dev)
        per = torch.empty((count, C.sizeof(itw_amd.RefineStats) // 8), dtype=torch.int64, device=dev)
        st, ist = itw_amd.RefineStats(), itw_amd.RefineStats()

        def chain(budget, bm=None, image_stats=None, arr=arr, n=count):
            ok = L.itwCompressImageChainRefined(C.cast(arr, C.c_void_p), n, out.data_ptr(), fcode, A, B, 7, budget, C.addressof(st), C.sizeof(st),
                                                image_stats.data_ptr() if image_stats is not None else None, bm.data_ptr() if bm is not None else None, None)
            assert ok, itw_amd.last_error()

        listed_loop = [0]

        def per_image(budget):                                   # what a caller does without the chain call
            total = 0
            for i in range(count):
                L.itwPadToMultipleOf4Device(C.byref(ssurf[i]), px, padded[i].data_ptr())
                ok = L.itwCompressImageRefined(C.byref(psurf[i]), out.data_ptr() + offs[i] * 16, fcode, A, B, 7, budget, C.addressof(ist), C.sizeof(ist), None, None)
                assert ok, itw_amd.last_error()
                total += int(ist.listed)
            listed_loop[0] = total

        def single(budget):
            ok = L.itwCompressImageRefined(C.byref(ssurf[0]), out.data_ptr(), fcode, A, B, 7, budget, C.addressof(ist), C.sizeof(ist), None, None)
            assert ok, itw_amd.last_error()

        def plain(settings):
            assert L.itwCompressImageChainEx(C.cast(arr, C.c_void_p), count, out.data_ptr(), fcode, C.addressof(settings), None, None)

        chain(U64_MAX, bmap)
        e = bmap.cpu().numpy()
        s = np.sort(e)
        budgets = {"10": int(s[nb - nb // 10 - 1]), "30": int(s[nb - (3 * nb) // 10 - 1])}
        variants = {"chain_first": lambda: plain(s1), "chain_refine": lambda: plain(s2)}
        for p, b in budgets.items():
            variants["per_image_" + p] = (lambda v: lambda: per_image(v))(b)
            variants["chain_" + p] = (lambda v: lambda: chain(v))(b)
            variants["chain_stats_" + p] = (lambda v: lambda: chain(v, None, per))(b)
        level0 = {}
        if faces == 1:                                           # level 0 alone: in place against packed
            s0 = np.sort(e[:nblocks[0]])
            n0 = nblocks[0]
            level0 = {"10": int(s0[n0 - n0 // 10 - 1]), "30": int(s0[n0 - (3 * n0) // 10 - 1])}
            one = (itw_amd.RgbaSurface * 1)(ssurf[0])
            for p, b in level0.items():
                variants["level0_single_" + p] = (lambda v: lambda: single(v))(b)
                variants["level0_chain_" + p] = (lambda v: lambda: chain(v, None, None, one, 1))(b)

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
        times = {k: [] for k in variants}
        for _ in range(reps):
            for k, fn in variants.items():
                times[k].append(timed(fn))
        row = {"case": name, "format": fmt, "first": first, "refine": refine, "top": [h, w], "faces": faces, "images": count, "blocks": nb,
               "reps": reps, "inner": inner, "timing": "host clock around calls that each end in a stream synchronise",
               "device": itw_amd.device_info(), "variants": {}}
        if label:
            row["build"] = label
        for k, fn in variants.items():
            t = sorted(times[k])
            v = {"ms": round(t[0], 4), "median_ms": round(t[len(t) // 2], 4), "spread": round((t[-1] - t[0]) / t[0], 3)}
            fn()
            if k.startswith("chain_1") or k.startswith("chain_3") or k.startswith("chain_stats") or k.startswith("level0_chain"):
                v.update(budget=(level0 if k.startswith("level0") else budgets)[k.rsplit("_", 1)[1]], listed=int(st.listed), replaced=int(st.replaced),
                         sse_first=int(st.sse_first), sse_final=int(st.sse_final))
            elif k.startswith("per_image"):
                v.update(budget=budgets[k.rsplit("_", 1)[1]], listed=listed_loop[0])
            elif k.startswith("level0_single"):
                v.update(budget=level0[k.rsplit("_", 1)[1]], listed=int(ist.listed), replaced=int(ist.replaced), sse_first=int(ist.sse_first),
                         sse_final=int(ist.sse_final))
            row["variants"][k] = v
        med = {k: row["variants"][k]["median_ms"] for k in variants}
        for p in budgets:
            row["chain_vs_per_image_" + p] = round(med["chain_" + p] / med["per_image_" + p], 3)
            row["image_stats_cost_ms_" + p] = round(med["chain_stats_" + p] - med["chain_" + p], 4)
        for p in level0:
            row["level0_chain_minus_single_ms_" + p] = round(med["level0_chain_" + p] - med["level0_single_" + p], 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if save and rows:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main_chain() if "--chain" in sys.argv else main_target() if "--target" in sys.argv else main()
