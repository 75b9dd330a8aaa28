"""What the height-map stage costs, device-resident (include/itw_dispatch.h, "height maps"): seeded heights of every source kind, 4096 x 4096
unless --size says otherwise.  One run: the legs alternate call by call, so that whatever the clocks do they do to all of them.  A call =
the entry point on device pointers followed by a synchronise of the stream, inside a host clock (time.perf_counter).  Per leg: the median of
reps x inner calls (default 7 x 5 = 35), the fastest call, p10 and p90.

Legs (K = int8, half, float; ops = red channel, wrap, occlusion, amplitude 2 unless said otherwise):
  h_K          the stage alone, out of place: itwQuantizeNormalMapChain with ITW_NORMAL_FROM_HEIGHT (also as a fraction of 8 TB/s over the
               source read once and the int8 image written)
  q_K          itwQuantizeNormalMapChain without the bit: a stream kernel over the same bytes with no neighbours
  p_rgba8, p_half      itwPrepareNormalMapChain with the bit, in place: the copy into the thread's buffer, then the stage
  n_rgba8, n_half      itwPrepareNormalMapChain without the bit (ops 7), in place, no copy
  copy_rgba8, copy_half     a device copy of the same image (hipMemcpy2DAsync through torch): what the scratch copy costs, and what the
               stage replaces as level 0 of itwCompressImageMipped
  m3, m3_height        itwCompressImageMipped to BC5 of a 1024^2 cube with mips, without and with the bit
  m4_K, m4_K_height    itwCompressSignedNormalMapMipped to BC5_SNORM of the same, without (the widening kernel) and with the bit

The rows labelled run1 / run2 in profiles/height_normal_timing.jsonl were recorded while a second kernel variant was still built (every
lane loading its own window, no LDS): their h_K_plain and p_*_plain legs are that variant's, measured in the same run through a second
copy of the library; it lost on every kind and was removed, and this tool no longer has those legs.

One JSON object per line (stdout, and appended to profiles/height_normal_timing.jsonl unless --no-save).
Usage: python tools/height_normal_timing.py [reps] [inner] [--size=N] [--label=TEXT] [--no-save] [--out=PATH]"""
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
KINDS = (("int8", 4), ("half", 8), ("float", 16))


def opt(name, default):
    return next((a[len(name) + 3:] for a in sys.argv if a.startswith("--" + name + "=")), default)


def heights(size):
    """float32 (size, size, 4) in [0, 1): smooth bumps plus noise"""
    rng = np.random.default_rng(3)
    y, x = np.mgrid[0:size, 0:size].astype(np.float32)
    bumps = (np.sin(x * np.float32(0.05)) * np.cos(y * np.float32(0.035)) * np.float32(0.35) + np.float32(0.5)).astype(np.float32)
    v = np.repeat(bumps[..., None], 4, axis=2) + rng.normal(0, 0.05, (size, size, 4)).astype(np.float32)
    return np.clip(v, 0, 1).astype(np.float32)


def as_kind(v, kind):
    if kind == "uint8":
        return np.rint(v * 255.0).astype(np.uint8)
    if kind == "int8":
        return np.rint(v * 127.0).astype(np.int8)
    return v.astype(np.float16).view(np.int16) if kind == "half" else np.ascontiguousarray(v, dtype=np.float32)


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    inner = int(args[1]) if len(args) > 1 else 5
    size = int(opt("size", 4096))
    out_path = opt("out", os.path.join(ROOT, "profiles", "height_normal_timing.jsonl"))
    OPS = itw_amd.height_ops("r", occlusion=True, amplitude=2.0)
    L = itw_amd.lib()
    S = itw_amd.RgbaSurface
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    L.itwSetStream(stream.cuda_stream)
    L.itwWarmupBC45()
    L.itwWarmupBC45S()

    v = heights(size)
    src = {k: torch.from_numpy(as_kind(v, k)).to(dev) for k in ("uint8", "int8", "half", "float")}
    surf = {k: S(src[k].data_ptr(), size, size, size * tb) for k, tb in KINDS + (("uint8", 4),)}
    scratch = torch.empty((size, size, 4), dtype=torch.int8, device=dev)
    s_scr = S(scratch.data_ptr(), size, size, size * 4)
    work = {"rgba8": src["uint8"].clone(), "half": src["half"].clone()}
    s_work = {"rgba8": S(work["rgba8"].data_ptr(), size, size, size * 4), "half": S(work["half"].data_ptr(), size, size, size * 8)}
    spare = {k: torch.empty_like(t) for k, t in work.items()}

    legs = []
    for k, tb in KINDS:
        s = surf[k]
        legs += [(f"h_{k}", lambda s=s, tb=tb: L.itwQuantizeNormalMapChain(C.byref(s), tb, C.byref(s_scr), 1, OPS)),
                 (f"q_{k}", lambda s=s, tb=tb: L.itwQuantizeNormalMapChain(C.byref(s), tb, C.byref(s_scr), 1, 7))]
    for k, px in (("rgba8", 4), ("half", 8)):
        sw = s_work[k]
        legs += [(f"p_{k}", lambda sw=sw, px=px: L.itwPrepareNormalMapChain(C.byref(sw), 1, px, OPS)),
                 (f"n_{k}", lambda sw=sw, px=px: L.itwPrepareNormalMapChain(C.byref(sw), 1, px, 7)),
                 (f"copy_{k}", lambda k=k: spare[k].copy_(work[k]))]
    keep = []
    if size >= 3072:                                              # six 1024^2 faces cut from the content
        def faces(t):
            return [t[(f // 3) * 1024:(f // 3) * 1024 + 1024, (f % 3) * 1024:(f % 3) * 1024 + 1024].contiguous() for f in range(6)]
        b8 = faces(src["uint8"])
        arr8 = itw_amd.abi._surfaces(b8)
        out3 = torch.empty(6 * sum(((max(1, 1024 >> l) + 3) // 4) ** 2 * 16 for l in range(11)), dtype=torch.uint8, device=dev)
        keep += [b8, arr8, out3]
        legs += [("m3", lambda: L.itwCompressImageMipped(C.cast(arr8, C.c_void_p), 6, 0, 4, out3.data_ptr(), 83, None, None, None)),
                 ("m3_height", lambda: L.itwCompressImageMipped(C.cast(arr8, C.c_void_p), 6, 0, OPS | 4, out3.data_ptr(), 83, None, None, None))]
        for k, tb in KINDS:
            bk = faces(src[k])
            arrk = (S * 6)(*[itw_amd.abi._signed_surface(b) for b in bk])
            keep += [bk, arrk]
            legs += [(f"m4_{k}", lambda arrk=arrk, tb=tb: L.itwCompressSignedNormalMapMipped(C.cast(arrk, C.c_void_p), 6, 0, tb, 4, out3.data_ptr(), 84, None, None)),
                     (f"m4_{k}_height", lambda arrk=arrk, tb=tb: L.itwCompressSignedNormalMapMipped(C.cast(arrk, C.c_void_p), 6, 0, tb, OPS | 4, out3.data_ptr(), 84, None, None))]

    for _ in range(3):                                            # warm-up: code objects, tables, the thread's buffers, clocks
        for _, call in legs:
            call()
    stream.synchronize()
    assert itw_amd.last_error() is None, itw_amd.last_error()
    times = {name: [] for name, _ in legs}
    for _ in range(reps):
        for _ in range(inner):
            for name, call in legs:                               # the legs alternate
                t0 = time.perf_counter()
                call()
                stream.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e6)
    row = {"size": size, "ops": OPS, "reps": reps, "inner": inner, "calls_per_leg": reps * inner, "label": opt("label", ""),
           "device": itw_amd.device_info(), "unit": "us per call, host clock around the call + stream synchronise"}
    for name, t in times.items():
        t = np.sort(np.array(t))
        row[name] = {"median_us": round(float(np.median(t)), 2), "min_us": round(float(t[0]), 2),
                     "p10_us": round(float(np.percentile(t, 10)), 2), "p90_us": round(float(np.percentile(t, 90)), 2)}
    med = lambda k: row[k]["median_us"]
    for k, tb in KINDS:
        row[f"h_{k}_fraction_of_8TBs"] = round(size * size * (tb + 4) / med(f"h_{k}") / PEAK_BYTES_PER_US, 3)
    for k, px in (("rgba8", 4), ("half", 8)):
        row[f"p_{k}_minus_copy_us"] = round(med(f"p_{k}") - med(f"copy_{k}"), 2)
        row[f"p_{k}_fraction_of_8TBs"] = round(size * size * px * 4 / med(f"p_{k}") / PEAK_BYTES_PER_US, 3)     # copy: read + write; stage: read + write
    print(json.dumps(row), flush=True)
    if "--no-save" not in sys.argv:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(json.dumps(row) + "\n")
    del keep


if __name__ == "__main__":
    main()
