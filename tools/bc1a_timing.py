"""BC1 with 1-bit alpha (DirectXTex's colour-key encoder, csrc/bc1a.hip) timed on the project's method: a call = the entry point followed by a
synchronise of its stream, inside a host clock (time.perf_counter); the legs of a group alternate call by call in one job, so that whatever
the clocks do they do to all of them; per leg the median of reps x inner calls (default 7 x 5 = 35), the fastest call and the spread
(p90 - p10) / median.  Run it twice and compare the rows: the difference between two runs is the noise floor of every comparison made here.

Groups (one JSON object per line on stdout, appended to profiles/bc1a_timing.jsonl unless --no-save):
  resident  4096^2 (--size=N) device-resident through itwCompressImageSlicedEx with one slice: BC1A plain, uniform, each dither bit, all
            flags; and, for scale, the ISPC BC1 kernel, BC3 and BC7 `alpha_basic` (what a cut-out had to be stored in before) through the
            same entry point.  Rows carry Mpix/s and, for BC1A, the share of HBM peak the traffic (4 B read per texel + 0.5 B written) comes to.
  sliced    the same surface from pageable host memory in 64 slices with a progress callback.
  mipped    a 1024^2 cube (six faces) with mips through compress_mipped(..., alpha_coverage=128), device-resident bases: bc1a, bc3, bc7 alpha_basic.
  builds    --lib=PATH: another build's libispc_texcomp.so (the parent commit's) against this one on BC1 and BC4, device-resident and sliced
            from host memory, alternating in the same job: the shared host layer.
Usage: python tools/bc1a_timing.py [reps] [inner] [--size=N] [--groups=resident,sliced,mipped,builds] [--lib=PATH] [--label=TEXT] [--no-save]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
import numpy as np                      # noqa: E402
import itw_amd                          # noqa: E402

HBM_PEAK_GBS = 8000.0                   # MI355X: 8 TB/s


def opt(name, default):
    return next((a[len(name) + 3:] for a in sys.argv if a.startswith("--" + name + "=")), default)


def summary(t):
    t = np.sort(np.array(t))
    med = float(np.median(t))
    return {"median_us": round(med, 1), "min_us": round(float(t[0]), 1), "spread": round(float(np.percentile(t, 90) - np.percentile(t, 10)) / med, 3)}


def alternate(legs, reps, inner, sync):
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


def cutout(size, seed=3):
    """Cut-out content: smooth colour with noise, an alpha plane of soft-rimmed discs over transparent ground."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:size, 0:size].astype(np.float32)
    img = np.empty((size, size, 4), dtype=np.uint8)
    img[..., 0] = (x * 255 / (size - 1)).astype(np.uint8)
    img[..., 1] = (y * 255 / (size - 1)).astype(np.uint8)
    img[..., 2] = rng.integers(0, 256, (size, size), dtype=np.uint8)
    a = np.zeros((size, size), dtype=np.float32)
    for _ in range(24):
        cy, cx, r = rng.uniform(0, size), rng.uniform(0, size), rng.uniform(size / 32, size / 6)
        a = np.maximum(a, np.clip((r - np.hypot(y - cy, x - cx)) / 3.0 + 0.5, 0, 1))
    img[..., 3] = np.rint(a * 255).astype(np.uint8)
    return img


def sliced_call(L, fmt, settings, surf, dst, width, slice_pixels, cb):
    sp = C.cast(C.byref(settings), C.c_void_p) if settings is not None else None
    pitch = itw_amd.block_count(fmt, width, 4) * itw_amd.BYTES_PER_BLOCK[itw_amd.abi._base(fmt)]
    code = itw_amd.DXGI_FORMAT[fmt]

    def call():
        assert L.itwCompressImageSlicedEx(C.byref(surf), dst, pitch, code, sp, slice_pixels, cb, None)
    return call


def legs_of(L, surf, dst, width, slice_pixels, cb, bc1a_only=False):
    S = itw_amd.Bc1aSettings
    legs = [("bc1a", "bc1a", S()), ("bc1a_uniform", "bc1a", S(uniform=True)), ("bc1a_dither_rgb", "bc1a", S(dither_rgb=True)),
            ("bc1a_dither_a", "bc1a", S(dither_a=True)), ("bc1a_all_flags", "bc1a", S(0.5, True, True, True))]
    if not bc1a_only:
        legs += [("bc1_ispc", "bc1", None), ("bc3", "bc3", None), ("bc7_alpha_basic", "bc7", itw_amd.bc7_profile("alpha_basic"))]
    return [(name, sliced_call(L, fmt, st, surf, dst, width, slice_pixels, cb)) for name, fmt, st in legs], [st for _, _, st in legs]


def main():
    import torch
    nums = [int(a) for a in sys.argv[1:] if a.isdigit()]
    reps, inner = nums[0] if nums else 7, nums[1] if len(nums) > 1 else 5
    size = int(opt("size", "4096"))
    groups = opt("groups", "resident,sliced,mipped").split(",")
    label = opt("label", "")
    out_path = os.path.join(ROOT, "profiles", "bc1a_timing.jsonl")
    L = itw_amd.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.itwSetStream(torch.cuda.current_stream(dev).cuda_stream)
    sync = torch.cuda.synchronize
    img = cutout(size)
    mpix = size * size / 1e6
    rows = []

    def row(group, name, s, extra=None):
        r = {"tool": "bc1a_timing", "group": group, "leg": name, "size": size, "reps": reps * inner, "label": label, "device": itw_amd.device_info(), **s,
             "mpix_s": round(mpix / (s["median_us"] * 1e-6), 1)}
        r.update(extra or {})
        rows.append(r)
        print(json.dumps(r), flush=True)

    if "resident" in groups:
        d_img = torch.from_numpy(img).to(dev)
        d_out = torch.empty(size * size, dtype=torch.uint8, device=dev)             # 16-byte blocks fit
        surf = itw_amd.RgbaSurface(d_img.data_ptr(), size, size, size * 4)
        legs, keep = legs_of(L, surf, d_out.data_ptr(), size, 1 << 62, None)
        for name, s in alternate(legs, reps, inner, sync).items():
            extra = {"hbm_share": round(size * size * 4.5 / (s["median_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)} if name.startswith("bc1a") else None
            row("resident", name, s, extra)
    if "sliced" in groups:
        out = np.empty(size * size, dtype=np.uint8)
        cb = itw_amd.PROGRESS_FUNC(lambda i, n, u: True)
        surf = itw_amd.RgbaSurface(img.ctypes.data, size, size, size * 4)
        legs, keep = legs_of(L, surf, out.ctypes.data, size, size * size // 64, C.cast(cb, C.c_void_p))
        for name, s in alternate(legs, reps, inner, sync).items():
            row("sliced_host_64", name, s)
    if "mipped" in groups:
        faces = [torch.from_numpy(cutout(1024, seed=10 + f)).to(dev) for f in range(6)]
        n = itw_amd.mip_levels(1024, 1024)
        outs = {f: torch.empty(6 * sum(((max(1, 1024 >> l) + 3) // 4) ** 2 for l in range(n)) * itw_amd.BYTES_PER_BLOCK[f], dtype=torch.uint8, device=dev)
                for f in ("bc1a", "bc3", "bc7")}
        a7 = itw_amd.bc7_profile("alpha_basic")
        s1 = itw_amd.Bc1aSettings(itw_amd.Bc1aSettings.ref_of(128))
        legs = [("bc1a", lambda: itw_amd.compress_mipped("bc1a", faces, alpha_coverage=128, settings=s1, out=outs["bc1a"])),
                ("bc3", lambda: itw_amd.compress_mipped("bc3", faces, alpha_coverage=128, out=outs["bc3"])),
                ("bc7_alpha_basic", lambda: itw_amd.compress_mipped("bc7", faces, alpha_coverage=128, settings=a7, out=outs["bc7"]))]
        for name, s in alternate(legs, reps, inner, sync).items():
            s["mpix_s"] = None
            rows.append({"tool": "bc1a_timing", "group": "mipped_cube_1024_coverage_128", "leg": name, "reps": reps * inner, "label": label, **s})
            print(json.dumps(rows[-1]), flush=True)
    other = opt("lib", "")
    if "builds" in groups and other:
        # the other build is bound by hand: it lacks what this build's package binds
        P = C.CDLL(other, mode=os.RTLD_LOCAL)
        for lib in (P, L):
            lib.itwCompressImageSlicedEx.argtypes = [C.POINTER(itw_amd.RgbaSurface), C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
            lib.itwCompressImageSlicedEx.restype = C.c_bool
        P.itwSetStream.argtypes = [C.c_void_p]
        P.itwSetStream(torch.cuda.current_stream(dev).cuda_stream)
        d_img = torch.from_numpy(img).to(dev)
        d_out = torch.empty(size * size, dtype=torch.uint8, device=dev)
        out = np.empty(size * size, dtype=np.uint8)
        cb = itw_amd.PROGRESS_FUNC(lambda i, n, u: True)
        dsurf = itw_amd.RgbaSurface(d_img.data_ptr(), size, size, size * 4)
        hsurf = itw_amd.RgbaSurface(img.ctypes.data, size, size, size * 4)
        legs = []
        for fmt in ("bc1", "bc4"):
            for build, lib in (("parent", P), ("this", L)):
                legs.append((f"{fmt}_resident_{build}", sliced_call(lib, fmt, None, dsurf, d_out.data_ptr(), size, 1 << 62, None)))
                legs.append((f"{fmt}_sliced_host_64_{build}", sliced_call(lib, fmt, None, hsurf, out.ctypes.data, size, size * size // 64, C.cast(cb, C.c_void_p))))
        for name, s in alternate(legs, reps, inner, sync).items():
            row("builds", name, s)
    if "--no-save" not in sys.argv and rows:
        with open(out_path, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
