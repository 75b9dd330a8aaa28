"""What mip generation costs (itwGenerateMipChain, itwCompressImageMipped; include/itw_dispatch.h "Mip chains"), in the method of
tools/normal_map_timing.py: a call = the entry point followed by a synchronise of the stream, inside a host clock (time.perf_counter);
the legs of a row alternate call by call in one run, so that whatever the clocks do they do to all of them; per leg the median of
reps x inner calls (default 7 x 5 = 35), the fastest call, p10 and p90 -- the run's own spread.

Rows (one JSON object per line; stdout, and appended to profiles/mipgen_timing.jsonl unless --no-save):
  2d_4096_rgba8 / _rgba16f, cube_1024_rgba8 / _rgba16f   full chains, device-resident: `pyramid` (the default route) against `per_level`
           (ITW_MIP_PER_LEVEL).  `bytes_per_level` = every level but the last read once and every level but the base written once: what the
           per-level route moves; `bytes_pyramid` = the base read and every other level written (levels +1 .. +5 of a tile never come back from
           memory; the one level a second launch re-reads is not counted).  Each leg's traffic over its median as a fraction of 8 TB/s
  linear_4000x3000_rgba16f                                the linear filter (one route)
  mipped_cube_1024_bc7_basic / _bc1                       the save path from six 1024^2 bases: itwCompressImageMipped from device bases
           (`mipped_device`, blocks to device memory) and from host bases (`mipped_host`, blocks to host memory), against what a caller does
           today with a chain made elsewhere (its making is not timed): itwCompressImageChainEx from host memory on the ready-made chain
           (`chain_host`: the whole chain goes up) and from device memory (`chain_device`)
Usage: python tools/mipgen_timing.py [reps] [inner] [--label=TEXT] [--no-save] [--out=PATH] [--only=SUBSTRING]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
import numpy as np                      # noqa: E402
import itw_amd                          # noqa: E402

PEAK_BYTES_PER_US = 8.0e6               # 8 TB/s


def opt(name, default):
    return next((a[len(name) + 3:] for a in sys.argv if a.startswith("--" + name + "=")), default)


def content(h, w, half, seed):
    rng = np.random.default_rng(seed)
    if half:
        return rng.random((h, w, 4), dtype=np.float32).astype(np.float16).view(np.int16)
    return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)


def measure(legs, reps, inner, stream):
    for _ in range(3):                                            # warm-up: code objects, the thread's buffers, clocks
        for _, call in legs:
            call()
    stream.synchronize()
    times = {name: [] for name, _ in legs}
    for _ in range(reps):
        for _ in range(inner):
            for name, call in legs:                               # the legs alternate
                t0 = time.perf_counter()
                call()
                stream.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e6)
    out = {}
    for name, t in times.items():
        t = np.sort(np.array(t))
        out[name] = {"median_us": round(float(np.median(t)), 2), "min_us": round(float(t[0]), 2),
                     "p10_us": round(float(np.percentile(t, 10)), 2), "p90_us": round(float(np.percentile(t, 90)), 2)}
    return out


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    inner = int(args[1]) if len(args) > 1 else 5
    only = opt("only", "")
    out_path = opt("out", os.path.join(ROOT, "profiles", "mipgen_timing.jsonl"))
    L = itw_amd.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    L.itwSetStream(stream.cuda_stream)

    def emit(row):
        row.update({"reps": reps, "inner": inner, "calls_per_leg": reps * inner, "label": opt("label", ""), "device": itw_amd.device_info(),
                    "unit": "us per call, host clock around the call + stream synchronise"})
        print(json.dumps(row), flush=True)
        if "--no-save" not in sys.argv:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "a") as f:
                f.write(json.dumps(row) + "\n")

    def device_chains(w, h, items, half):
        n = itw_amd.mip_levels(w, h)
        chains = []
        for i in range(items):
            base = torch.from_numpy(content(h, w, half, 10 + i)).to(dev)
            chains.append([base] + [torch.empty((max(1, h >> l), max(1, w >> l), 4), dtype=base.dtype, device=dev) for l in range(1, n)])
        return chains, n

    for name, w, h, items, half in (("2d_4096_rgba8", 4096, 4096, 1, False), ("2d_4096_rgba16f", 4096, 4096, 1, True),
                                    ("cube_1024_rgba8", 1024, 1024, 6, False), ("cube_1024_rgba16f", 1024, 1024, 6, True),
                                    ("linear_4000x3000_rgba16f", 4000, 3000, 1, True)):
        if only not in name:
            continue
        chains, n = device_chains(w, h, items, half)
        px = 8 if half else 4
        arr = C.cast(itw_amd.abi._surfaces([lv for ch in chains for lv in ch]), C.c_void_p)
        sizes = [max(1, w >> l) * max(1, h >> l) * px for l in range(n)]
        traffic = items * sum(sizes[l - 1] + sizes[l] for l in range(1, n))
        least = items * sum(sizes)
        linear = name.startswith("linear")
        legs = [("linear" if linear else "pyramid", lambda: L.itwGenerateMipChain(arr, items, n, px, 0))]
        if not linear:
            legs.append(("per_level", lambda: L.itwGenerateMipChain(arr, items, n, px, itw_amd.MIP_PER_LEVEL)))
        row = {"row": name, "width": w, "height": h, "items": items, "levels": n, "pixel_size": px, "bytes_per_level": traffic, "bytes_pyramid": least}
        row.update(measure(legs, reps, inner, stream))
        for leg, _ in legs:
            row[leg + "_fraction_of_8TBs"] = round((least if leg == "pyramid" else traffic) / row[leg]["median_us"] / PEAK_BYTES_PER_US, 3)
        if not linear:
            row["pyramid_over_per_level"] = round(row["pyramid"]["median_us"] / row["per_level"]["median_us"], 3)
        emit(row)
        del chains

    for fmt, profile in (("bc7", "basic"), ("bc1", None)):
        name = "mipped_cube_1024_" + fmt + ("_" + profile if profile else "")
        if only not in name:
            continue
        w = h = 1024
        chains, n = device_chains(w, h, 6, False)
        itw_amd.generate_mips_into(chains)
        stream.synchronize()
        flat_dev = [lv for ch in chains for lv in ch]
        flat_host = [lv.cpu().numpy() for lv in flat_dev]                       # the ready-made chain of the comparison legs
        bases_dev = C.cast(itw_amd.abi._surfaces([ch[0] for ch in chains]), C.c_void_p)
        bases_host = C.cast(itw_amd.abi._surfaces([flat_host[i * n] for i in range(6)]), C.c_void_p)
        arr_dev, arr_host = C.cast(itw_amd.abi._surfaces(flat_dev), C.c_void_p), C.cast(itw_amd.abi._surfaces(flat_host), C.c_void_p)
        nbytes = itw_amd.chain_bytes(fmt, flat_dev)
        out_dev = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out_host = np.empty(nbytes, dtype=np.uint8)
        settings = itw_amd.bc7_profile(profile) if fmt == "bc7" else None
        sp = C.cast(C.byref(settings), C.c_void_p) if settings is not None else None
        code = itw_amd.DXGI_FORMAT[fmt]
        legs = [("mipped_device", lambda: L.itwCompressImageMipped(bases_dev, 6, 0, 0, out_dev.data_ptr(), code, sp, None, None)),
                ("mipped_host", lambda: L.itwCompressImageMipped(bases_host, 6, 0, 0, out_host.ctypes.data, code, sp, None, None)),
                ("chain_host", lambda: L.itwCompressImageChainEx(arr_host, 6 * n, out_host.ctypes.data, code, sp, None, None)),
                ("chain_device", lambda: L.itwCompressImageChainEx(arr_dev, 6 * n, out_dev.data_ptr(), code, sp, None, None))]
        row = {"row": name, "width": w, "height": h, "items": 6, "levels": n, "format": fmt, "profile": profile or "", "stream_bytes": nbytes}
        row.update(measure(legs, reps, inner, stream))
        row["mipped_host_over_chain_host"] = round(row["mipped_host"]["median_us"] / row["chain_host"]["median_us"], 3)
        row["mipped_device_over_chain_device"] = round(row["mipped_device"]["median_us"] / row["chain_device"]["median_us"], 3)
        emit(row)


if __name__ == "__main__":
    main()
