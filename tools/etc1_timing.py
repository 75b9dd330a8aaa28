"""ETC1 at fastSkipTreshold 1, 6 and 32 against BC1 and BC7 `basic` of the same build, device-resident 4096^2 (or --size=N), one run: the
legs alternate call by call, so that whatever the clocks do they do to all of them.

A call = the entry point on device pointers followed by a synchronise of its stream, inside a host clock (time.perf_counter): what a
caller waiting for the blocks sees.  Everything is warmed up first.  Per leg: the median of reps x inner calls (default 7 x 5 = 35), the
fastest call, and the spread as (p90 - p10) / median.

For scale, the reference library's time for the same surface cut to 512^2 (oracle/_ref/libispc_texcomp_ref_full.so, where build() made
it): 16 host threads over row bands, one call per threshold.  That library is a SCALAR build of the reference, not ISPC SIMD: it says what
the checker costs, not what the reference's shipped object code would.

One JSON object per line (stdout, and appended to profiles/etc1_timing.jsonl unless --no-save).
Usage: python tools/etc1_timing.py [reps] [inner] [--size=N] [--label=TEXT] [--no-save] [--out=PATH] [--no-reference]

Above the block call (rows go to profiles/etc1_chain_timing.jsonl; same clock, same medians of reps x inner calls, legs alternating):
  --chain   itwCompressImageChainEx at the `slow` preset against the per-image loop of pad + itwCompressBlocksETC1 (each call followed
            by a synchronise, as the plugin's loop blocks per image): the 1024^2 cube map with mips (66 images) and the 2048^2 2D chain,
            device-resident (the loop's padded images are made once, outside the clock) and from host memory (the loop pads inside it).
  --sliced  4096^2 in 64 slices from pageable host memory with a progress callback: the pipeline (itwCompressImageSlicedEx), the
            literal loop (itwSetSliceWindow(-1), itwCompressImageSliced with a caller's function around itwCompressBlocksETC1 -- a
            ctypes callback, 64 calls of a few microseconds) and one itwCompressBlocksETC1 call over the surface.
  --bc7     BC7 `basic` through the code ETC1 now shares: the chain call on the two chains above (host and device) and the 64-slice
            pipeline, for comparing two builds.  --lib=PATH loads another build's libispc_texcomp.so (bound here by hand: an older
            build lacks symbols the package binds); --build=TEXT names it in the row."""
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
import numpy as np                      # noqa: E402
import itw_amd                          # noqa: E402
from itw_amd import surfaces           # noqa: E402

THRESHOLDS = (1, 6, 32)
REF_THREADS = 16


def opt(name, default):
    return next((a[len(name) + 3:] for a in sys.argv if a.startswith("--" + name + "=")), default)


def reference_leg(img):
    """ms per 512^2 call of the reference library at each threshold, on REF_THREADS host threads by row bands; None where it is not built"""
    path = os.path.join(ROOT, "oracle", "_ref", "libispc_texcomp_ref_full.so")
    if not os.path.exists(path):
        return None
    R = C.CDLL(path, mode=os.RTLD_LOCAL)
    h, w = img.shape[:2]
    rows = [(h // 4) * i // REF_THREADS * 4 for i in range(REF_THREADS + 1)]
    out = np.zeros((h // 4) * (w // 4) * 8, dtype=np.uint8)
    res = {}
    for t in THRESHOLDS:
        st = itw_amd.EtcSettings(t)

        def band(i):
            surf = itw_amd.RgbaSurface(img.ctypes.data + rows[i] * img.strides[0], w, rows[i + 1] - rows[i], img.strides[0])
            R.CompressBlocksETC1(C.byref(surf), C.c_void_p(out.ctypes.data + (rows[i] // 4) * (w // 4) * 8), C.byref(st))

        t0 = time.perf_counter()
        with ThreadPoolExecutor(REF_THREADS) as ex:
            list(ex.map(band, range(REF_THREADS)))
        res[f"t{t}_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    return res


def summary(t):
    t = np.sort(np.array(t))
    med = float(np.median(t))
    return {"median_us": round(med, 1), "min_us": round(float(t[0]), 1), "spread": round(float(np.percentile(t, 90) - np.percentile(t, 10)) / med, 3)}


def alternate(legs, reps, inner, sync):
    """legs: [(name, fn)].  Warm-up, then reps x inner rounds with the legs alternating call by call; {name: summary}."""
    for _ in range(2):
        for _, fn in legs:
            fn()
            sync()
    times = {name: [] for name, _ in legs}
    for _ in range(reps * inner):
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            sync()
            times[name].append((time.perf_counter() - t0) * 1e6)
    return {name: summary(t) for name, t in times.items()}


CHAINS = (("1024_cube", 1024, 6), ("2048_2d", 2048, 1))


def chain_images(size, faces):
    return [lv for f in range(faces) for lv in itw_amd.mip_chain(surfaces.ldr_smooth(size, size, seed=100 + f))]


def surfaces_of(items):
    """ctypes array of rgba_surface over numpy arrays / CUDA tensors"""
    s = [itw_amd.RgbaSurface(t.data_ptr(), t.shape[1], t.shape[0], t.stride(0)) if hasattr(t, "data_ptr")
         else itw_amd.RgbaSurface(t.ctypes.data, t.shape[1], t.shape[0], t.strides[0]) for t in items]
    return (itw_amd.RgbaSurface * len(s))(*s)


def emit(rows, out_path):
    for row in rows:
        print(json.dumps(row), flush=True)
    if "--no-save" not in sys.argv and rows:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


def chain_mode(reps, inner, out_path):
    import torch
    L = itw_amd.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.itwSetStream(torch.cuda.current_stream(dev).cuda_stream)
    sync = torch.cuda.synchronize
    st = itw_amd.etc_profile("slow")
    sp = C.cast(C.byref(st), C.c_void_p)
    rows = []
    for name, size, faces in CHAINS:
        images = chain_images(size, faces)
        offs = np.concatenate([[0], np.cumsum([((lv.shape[0] + 3) // 4) * ((lv.shape[1] + 3) // 4) * 8 for lv in images])]).astype(np.int64)
        nbytes = int(offs[-1])
        for where in ("device", "host"):
            if where == "device":
                srcs = [torch.from_numpy(lv).to(dev) for lv in images]
                padded = [torch.from_numpy(itw_amd.pad_to_multiple_of_4(lv)).to(dev) for lv in images]
                out_chain, out_loop = (torch.zeros(nbytes, dtype=torch.uint8, device=dev) for _ in range(2))
                dst_chain, dst_loop = out_chain.data_ptr(), out_loop.data_ptr()
                psurf = surfaces_of(padded)

                def loop():
                    for i in range(len(images)):
                        L.itwCompressBlocksETC1(C.byref(psurf[i]), dst_loop + int(offs[i]), C.byref(st))
                        sync()
            else:
                srcs = images
                out_chain, out_loop = np.zeros(nbytes, np.uint8), np.zeros(nbytes, np.uint8)
                dst_chain, dst_loop = out_chain.ctypes.data, out_loop.ctypes.data

                def loop():
                    for i, lv in enumerate(images):
                        src = itw_amd.pad_to_multiple_of_4(lv) if (lv.shape[0] % 4 or lv.shape[1] % 4) else lv
                        s = itw_amd.RgbaSurface(src.ctypes.data, src.shape[1], src.shape[0], src.strides[0])
                        L.itwCompressBlocksETC1(C.byref(s), dst_loop + int(offs[i]), C.byref(st))
            arr = surfaces_of(srcs)

            def chain():
                assert L.itwCompressImageChainEx(C.cast(arr, C.c_void_p), len(srcs), dst_chain, itw_amd.DXGI_FORMAT["etc1"], sp, None, None)

            res = alternate([("chain", chain), ("per_image", loop)], reps, inner, sync)
            a = out_chain.cpu().numpy() if hasattr(out_chain, "cpu") else out_chain
            b = out_loop.cpu().numpy() if hasattr(out_loop, "cpu") else out_loop
            rows.append({"mode": "chain", "case": "etc1_slow_" + name, "pointers": where, "images": len(images), "blocks": nbytes // 8,
                         "calls_per_leg": reps * inner, **res, "per_image_over_chain": round(res["per_image"]["median_us"] / res["chain"]["median_us"], 2),
                         "bytes_equal": bool(np.array_equal(a, b)), "label": opt("label", ""), "device": L.itwDeviceInfo().decode(),
                         "unit": "us per chain, host clock around the call(s) + synchronise"})
    emit(rows, out_path)
    return all(r["bytes_equal"] for r in rows)


def sliced_mode(reps, inner, out_path):
    L = itw_amd.lib()
    size = int(opt("size", 4096))
    img = surfaces.ldr_smooth(size, size)
    st = itw_amd.etc_profile("slow")
    sp = C.cast(C.byref(st), C.c_void_p)
    nbytes = (size // 4) ** 2 * 8
    outs = {k: np.zeros(nbytes, np.uint8) for k in ("pipeline", "literal_loop", "one_call")}
    surf = itw_amd.RgbaSurface(img.ctypes.data, size, size, img.strides[0])
    code, pitch = itw_amd.DXGI_FORMAT["etc1"], (size // 4) * 8
    calls = []
    cb = itw_amd.PROGRESS_FUNC(lambda i, n, u: calls.append(i) or True)
    own = itw_amd.abi.COMPRESSION_FUNC(lambda s, o: L.itwCompressBlocksETC1(s, o, C.byref(st)))

    def pipeline():
        L.itwSetSliceWindow(0)
        assert L.itwCompressImageSlicedEx(C.byref(surf), outs["pipeline"].ctypes.data, pitch, code, sp, 0, C.cast(cb, C.c_void_p), None)

    def literal():
        L.itwSetSliceWindow(-1)
        assert L.itwCompressImageSliced(C.byref(surf), outs["literal_loop"].ctypes.data, pitch, C.cast(own, C.c_void_p), code, False, 0, C.cast(cb, C.c_void_p), None)
        L.itwSetSliceWindow(0)

    def one():
        L.itwCompressBlocksETC1(C.byref(surf), outs["one_call"].ctypes.data, C.byref(st))

    res = alternate([("pipeline", pipeline), ("literal_loop", literal), ("one_call", one)], reps, inner, lambda: None)      # host pointers: every call is synchronous
    slices = max(1, size * size // 0x40000)
    row = {"mode": "sliced", "case": f"etc1_slow_{size}", "slices": slices, "window_slices": int(L.itwSliceWindowFor(code, sp, size, size, 0)),
           "progress_calls_per_call": len(calls) // (2 * (reps * inner + 2)), "calls_per_leg": reps * inner, **res,
           "literal_loop_over_pipeline": round(res["literal_loop"]["median_us"] / res["pipeline"]["median_us"], 2),
           "one_call_over_pipeline": round(res["one_call"]["median_us"] / res["pipeline"]["median_us"], 2),
           "bytes_equal": bool(np.array_equal(outs["pipeline"], outs["one_call"]) and np.array_equal(outs["literal_loop"], outs["one_call"])),
           "label": opt("label", ""), "device": L.itwDeviceInfo().decode(), "unit": "us per 4096^2 surface, host clock, pageable host memory, progress callback"}
    emit([row], out_path)
    return row["bytes_equal"]


def bc7_mode(reps, inner, out_path):
    """BC7 `basic` chain and sliced rows of one build (--lib=PATH, --build=TEXT)"""
    import torch
    path = opt("lib", itw_amd.lib_path())
    L = C.CDLL(path, mode=C.RTLD_LOCAL)
    L.itwCompressImageChainEx.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.itwCompressImageChainEx.restype = C.c_bool
    L.itwCompressImageSliced.argtypes = [C.POINTER(itw_amd.RgbaSurface), C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_bool, C.c_int64, C.c_void_p, C.c_void_p]
    L.itwCompressImageSliced.restype = C.c_bool
    L.itwSetStream.argtypes = [C.c_void_p]
    L.itwSetStream.restype = None
    L.itwDeviceInfo.restype = C.c_char_p
    basic = itw_amd.Bc7Settings()
    L.GetProfile_basic(C.byref(basic))
    sp = C.cast(C.byref(basic), C.c_void_p)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.itwSetStream(torch.cuda.current_stream(dev).cuda_stream)
    sync = torch.cuda.synchronize
    legs, keep = [], []
    for name, size, faces in CHAINS:
        images = chain_images(size, faces)
        nbytes = sum(((lv.shape[0] + 3) // 4) * ((lv.shape[1] + 3) // 4) * 16 for lv in images)
        for where in ("device", "host"):
            srcs = [torch.from_numpy(lv).to(dev) for lv in images] if where == "device" else images
            out = torch.zeros(nbytes, dtype=torch.uint8, device=dev) if where == "device" else np.zeros(nbytes, np.uint8)
            arr = surfaces_of(srcs)
            keep.append((srcs, out, arr))
            dst = out.data_ptr() if where == "device" else out.ctypes.data
            legs.append((f"chain_{name}_{where}", (lambda arr=arr, n=len(srcs), dst=dst: L.itwCompressImageChainEx(C.cast(arr, C.c_void_p), n, dst, 98, sp, None, None))))
    img = surfaces.ldr_smooth(4096, 4096)
    out = np.zeros(1024 * 1024 * 16, np.uint8)
    surf = itw_amd.RgbaSurface(img.ctypes.data, 4096, 4096, img.strides[0])
    cb = itw_amd.PROGRESS_FUNC(lambda i, n, u: True)
    fn = C.cast(L.CompressImageBC7_basic, C.c_void_p)
    legs.append(("sliced_4096_64", lambda: L.itwCompressImageSliced(C.byref(surf), out.ctypes.data, 1024 * 16, fn, 98, False, 0, C.cast(cb, C.c_void_p), None)))
    res = alternate(legs, reps, inner, sync)
    import hashlib
    sha = hashlib.sha256(out.tobytes()).hexdigest()[:16]
    emit([{"mode": "bc7_basic", "build": opt("build", ""), "lib": os.path.relpath(path, ROOT), "calls_per_leg": reps * inner, **res,
           "sliced_sha256_16": sha, "label": opt("label", ""), "device": L.itwDeviceInfo().decode(), "unit": "us per call, host clock around call + synchronise"}], out_path)
    return True


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    inner = int(args[1]) if len(args) > 1 else 5
    for flag, mode in (("--chain", chain_mode), ("--sliced", sliced_mode), ("--bc7", bc7_mode)):
        if flag in sys.argv:
            ok = mode(reps, inner, opt("out", os.path.join(ROOT, "profiles", "etc1_chain_timing.jsonl")))
            sys.exit(0 if ok else 1)
    size = int(opt("size", 4096))
    out_path = opt("out", os.path.join(ROOT, "profiles", "etc1_timing.jsonl"))
    L = itw_amd.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    L.itwSetStream(stream.cuda_stream)
    img = surfaces.ldr_smooth(size, size)
    src = torch.from_numpy(img).to(dev)
    surf = itw_amd.RgbaSurface(src.data_ptr(), size, size, size * 4)
    blocks = (size // 4) ** 2
    out8 = torch.empty(blocks * 8, dtype=torch.uint8, device=dev)
    out16 = torch.empty(blocks * 16, dtype=torch.uint8, device=dev)
    basic = itw_amd.bc7_profile("basic")
    etc = {t: itw_amd.EtcSettings(t) for t in THRESHOLDS}
    calls = [(f"etc1_t{t}", (lambda t=t: L.itwCompressBlocksETC1(C.byref(surf), out8.data_ptr(), C.byref(etc[t])))) for t in THRESHOLDS]
    calls.append(("bc1", lambda: L.CompressBlocksBC1(C.byref(surf), out8.data_ptr())))
    calls.append(("bc7_basic", lambda: L.CompressBlocksBC7(C.byref(surf), out16.data_ptr(), C.byref(basic))))
    for _ in range(3):                                            # warm-up: code objects, workspace, clocks
        for _, fn in calls:
            fn()
    stream.synchronize()
    times = {name: [] for name, _ in calls}
    for _ in range(reps):
        for _ in range(inner):
            for name, fn in calls:                                # the legs alternate
                t0 = time.perf_counter()
                fn()
                stream.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e6)
    row = {"size": size, "reps": reps, "inner": inner, "calls_per_leg": reps * inner, "label": opt("label", ""),
           "device": L.itwDeviceInfo().decode(), "unit": "us per call, host clock around call + stream synchronise"}
    for name, t in times.items():
        t = np.sort(np.array(t))
        med = float(np.median(t))
        row[name] = {"median_us": round(med, 1), "min_us": round(float(t[0]), 1),
                     "spread": round(float(np.percentile(t, 90) - np.percentile(t, 10)) / med, 3),
                     "mpix_per_s": round(size * size / med, 1)}
    for t in THRESHOLDS:
        row[f"etc1_t{t}_over_bc7_basic"] = round(row[f"etc1_t{t}"]["median_us"] / row["bc7_basic"]["median_us"], 2)
    if "--no-reference" not in sys.argv:
        cut = min(512, size)
        ref = reference_leg(np.ascontiguousarray(img[:cut, :cut]))
        row["reference_512"] = ({"what": f"scalar build of the reference, not ISPC SIMD; {cut}^2 cut of the same surface, {REF_THREADS} host threads by row bands, one call",
                                 **ref} if ref else "oracle/_ref is not built here: not measured")
    print(json.dumps(row), flush=True)
    if "--no-save" not in sys.argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
