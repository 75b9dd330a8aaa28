"""A whole mip chain / cube map in one call (itwCompressImageChainEx) against the plugin's per-image pattern (IntelPlugin.cpp:229-255: per
image, the pad to multiples of 4 when the size needs it, then itwCompressImageSliced with the matching trampoline and 0x40000-pixel
slices).  Every case runs with host pointers (what the plugin passes; the per-image pattern pads on the host inside the timed loop) and
device-resident (images and target on the device; the per-image pattern's padded images are made once, outside the timed loop).
Warm-up, then best and median of `reps` runs and their spread; the two outputs are compared byte for byte.
One JSON object per line (stdout, and appended to profiles/chain_timing.jsonl unless --no-save).
Usage: python tools/chain_timing.py [reps] [case,case,...] [--no-save] [--out=PATH] [--chain-only] (the chain call alone: for a kernel trace)"""
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

# name, format, profile, top size (h, w), faces
CASES = [("bc7_basic_2048_2d", "bc7", "basic", (2048, 2048), 1),
         ("bc7_basic_1024_cube", "bc7", "basic", (1024, 1024), 6),
         ("bc7_slow_1023x517_2d", "bc7", "slow", (1023, 517), 1),
         ("bc1_4096_2d", "bc1", None, (4096, 4096), 1),
         ("bc3_4096_2d", "bc3", None, (4096, 4096), 1),
         ("bc6h_slow_512_cube", "bc6h", "slow", (512, 512), 6),
         ("bc4_1024_2d", "bc4", None, (1024, 1024), 1),
         ("bc5_1024_2d", "bc5", None, (1024, 1024), 1)]


def timed(fn, reps, sync):
    fn(); sync()                          # warm (first calls size the staging buffers)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn(); sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[0], ts[len(ts) // 2], (ts[-1] - ts[0]) / ts[0]


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 10
    only = args[1].split(",") if len(args) > 1 else None
    save = "--no-save" not in sys.argv
    chain_only = "--chain-only" in sys.argv
    out_path = next((a[6:] for a in sys.argv if a.startswith("--out=")), os.path.join(ROOT, "profiles", "chain_timing.jsonl"))
    L = itw_amd.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    sync = torch.cuda.synchronize
    rows = []
    for name, fmt, prof, (h, w), faces in CASES:
        if only and name not in only:
            continue
        gen = surfaces.hdr_smooth if fmt == "bc6h" else surfaces.ldr_smooth
        images = [lv for f in range(faces) for lv in itw_amd.mip_chain(gen(h, w, seed=100 + f))]
        nbytes = itw_amd.chain_bytes(fmt, images)
        blocks = nbytes // itw_amd.BYTES_PER_BLOCK[fmt]
        pad = fmt not in itw_amd.KEEPS_PARTIAL_BLOCKS
        fn = itw_amd.image_func(fmt, prof)
        fcode = itw_amd.DXGI_FORMAT[fmt]
        settings = itw_amd.bc7_profile(prof) if fmt == "bc7" else (itw_amd.bc6h_profile(prof) if fmt == "bc6h" else None)
        sp = C.cast(C.byref(settings), C.c_void_p) if settings is not None else None
        offs = np.concatenate([[0], np.cumsum([((lv.shape[0] + 3) // 4) * ((lv.shape[1] + 3) // 4) * itw_amd.BYTES_PER_BLOCK[fmt] for lv in images])])

        for where in ("host", "device"):
            if where == "host":
                srcs = images
                out_chain = np.zeros(nbytes, np.uint8)
                out_loop = np.zeros(nbytes, np.uint8)
                dst_chain, dst_loop = out_chain.ctypes.data, out_loop.ctypes.data
                arr = (itw_amd.RgbaSurface * len(srcs))(*[itw_amd.RgbaSurface(lv.ctypes.data, lv.shape[1], lv.shape[0], lv.strides[0]) for lv in srcs])
                def loop():
                    for i, lv in enumerate(images):
                        src = itw_amd.pad_to_multiple_of_4(lv) if pad and (lv.shape[0] % 4 or lv.shape[1] % 4) else lv
                        s = itw_amd.RgbaSurface(src.ctypes.data, src.shape[1], src.shape[0], src.strides[0])
                        pitch = itw_amd.block_count(fmt, src.shape[1], 4) * itw_amd.BYTES_PER_BLOCK[fmt]
                        L.itwCompressImageSliced(C.byref(s), dst_loop + int(offs[i]), pitch, fn, fcode, True, 0, None, None)
            else:
                srcs = [torch.from_numpy(lv).to(dev) for lv in images]
                padded = [torch.from_numpy(itw_amd.pad_to_multiple_of_4(lv) if pad else lv).to(dev) for lv in images]
                out_chain = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
                out_loop = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
                dst_chain, dst_loop = out_chain.data_ptr(), out_loop.data_ptr()
                arr = (itw_amd.RgbaSurface * len(srcs))(*[itw_amd.RgbaSurface(t.data_ptr(), t.shape[1], t.shape[0], t.stride(0) * t.element_size()) for t in srcs])
                psurf = [itw_amd.RgbaSurface(t.data_ptr(), t.shape[1], t.shape[0], t.stride(0) * t.element_size()) for t in padded]
                L.itwSetStream(torch.cuda.current_stream(dev).cuda_stream)
                sync()

                def loop():
                    for i, s in enumerate(psurf):
                        pitch = itw_amd.block_count(fmt, s.width, 4) * itw_amd.BYTES_PER_BLOCK[fmt]
                        L.itwCompressImageSliced(C.byref(s), dst_loop + int(offs[i]), pitch, fn, fcode, True, 0, None, None)

            def chain():
                assert L.itwCompressImageChainEx(C.cast(arr, C.c_void_p), len(srcs), dst_chain, fcode, sp, None, None)

            c_best, c_med, c_spread = timed(chain, reps, sync)
            if chain_only:
                print(json.dumps({"case": name, "pointers": where, "chain_ms": round(c_best, 3), "images": len(images)}), flush=True)
                continue
            l_best, l_med, l_spread = timed(loop, reps, sync)
            a = out_chain.cpu().numpy() if hasattr(out_chain, "cpu") else out_chain
            b = out_loop.cpu().numpy() if hasattr(out_loop, "cpu") else out_loop
            row = {"case": name, "pointers": where, "format": fmt, "profile": prof, "top": [h, w], "faces": faces, "images": len(images),
                   "blocks": int(blocks), "chain_ms": round(c_best, 3), "chain_median_ms": round(c_med, 3), "chain_spread": round(c_spread, 3),
                   "per_image_ms": round(l_best, 3), "per_image_median_ms": round(l_med, 3), "per_image_spread": round(l_spread, 3),
                   "speedup": round(l_best / c_best, 2), "bytes_equal": bool(np.array_equal(a, b)), "reps": reps,
                   "device": itw_amd.device_info()}
            print(json.dumps(row), flush=True)
            rows.append(row)
    if save and rows:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if not all(r["bytes_equal"] for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
