"""itwMeasureBlocks (decode + compare + reduce in one kernel) against the route that existed before it: itwDecodeBlocks into a device
surface, then the torch reduction of tests/test_gpu_decode.py::_psnr (float difference, square, mean, .item()).  4096^2, everything
device-resident: BC1, BC7 (a `basic` stream of surfaces.ldr_smooth) and BC6H (a `basic` stream of surfaces.hdr_smooth).
Timed with device events around `inner` back-to-back calls after a warm-up, the routes alternating within each repetition; best and
median of `reps` repetitions per call.  The torch route ends in .item(), a host read-back, so the fused call is also timed through the
binding's measure(), which reads its 216 bytes back.  The fused call's bytes are the ones the algorithm needs -- the blocks and the source texels once --
over its time.  One JSON object per line (stdout, and appended to profiles/measure_timing.jsonl unless --no-save).
Usage: python tools/measure_timing.py [reps] [inner] [--no-save] [--out=PATH] [--size=N]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
import numpy as np                      # noqa: E402
import itw_amd                          # noqa: E402
from itw_amd import surfaces           # noqa: E402

CASES = [("bc1", None), ("bc7", "basic"), ("bc6h", "basic")]


def _psnr(a, b):                          # tests/test_gpu_decode.py::_psnr, as it stands
    import torch
    mse = torch.mean((a.float() - b.float()) ** 2).item()
    return 10 * np.log10(255.0 ** 2 / max(mse, 1e-12))


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 10
    inner = int(args[1]) if len(args) > 1 else 10
    save = "--no-save" not in sys.argv
    size = int(next((a[7:] for a in sys.argv if a.startswith("--size=")), 4096))
    out_path = next((a[6:] for a in sys.argv if a.startswith("--out=")), os.path.join(ROOT, "profiles", "measure_timing.jsonl"))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rows = []
    for fmt, prof in CASES:
        hdr = fmt == "bc6h"
        img = torch.from_numpy((surfaces.hdr_smooth(size, size).view(np.int16)) if hdr else surfaces.ldr_smooth(size, size)).to(dev)
        blocks = itw_amd.compress(fmt, img, prof)
        torch.cuda.synchronize()
        nblocks = (size // 4) ** 2
        raw = torch.zeros(C.sizeof(itw_amd.ErrorStats), dtype=torch.uint8, device=dev)
        channels = 3 if fmt in ("bc1", "bc6h") else 4

        def fused():
            itw_amd.measure_async(fmt, blocks, img, raw)

        def fused_read_back():                                  # the binding's measure(): allocates the 216 bytes, copies them to the host
            return itw_amd.measure(fmt, blocks, img)

        def two_step():
            dec = itw_amd.decode(fmt, blocks, size, size)
            return _psnr(dec[..., :channels], img[..., :channels])

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / inner

        for _ in range(3):                                       # warm-up: code objects, torch's allocator
            fused(); two_step(); fused_read_back()
        torch.cuda.synchronize()
        tf, tt, tr = [], [], []
        for _ in range(reps):
            tf.append(timed(fused))
            tt.append(timed(two_step))
            tr.append(timed(fused_read_back))
        tf.sort(); tt.sort(); tr.sort()
        st = itw_amd.stats_from_tensor(raw)
        bytes_needed = nblocks * itw_amd.BYTES_PER_BLOCK[fmt] + size * size * (8 if hdr else 4)
        row = {"format": fmt, "profile": prof, "size": size, "blocks": nblocks, "reps": reps, "inner": inner,
               "measure_ms": round(tf[0], 4), "measure_median_ms": round(tf[len(tf) // 2], 4), "measure_spread": round((tf[-1] - tf[0]) / tf[0], 3),
               "measure_read_back_ms": round(tr[0], 4), "measure_read_back_median_ms": round(tr[len(tr) // 2], 4),
               "decode_then_torch_ms": round(tt[0], 4), "decode_then_torch_median_ms": round(tt[len(tt) // 2], 4),
               "decode_then_torch_spread": round((tt[-1] - tt[0]) / tt[0], 3),
               "measure_bytes": bytes_needed, "measure_GBps": round(bytes_needed / (tf[0] * 1e-3) / 1e9, 1),
               "speedup": round(tt[0] / tf[0], 2), "measure_is_faster": bool(tf[0] < tt[0] and tf[len(tf) // 2] < tt[len(tt) // 2]),
               "sse": [int(v) for v in st.sse], "device": itw_amd.device_info()}
        if not hdr:
            row["psnr_db"] = round(st.psnr("rgb" if channels == 3 else "rgba"), 4)
            row["torch_psnr_db"] = round(float(two_step()), 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if save and rows:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if not all(r["measure_is_faster"] for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
