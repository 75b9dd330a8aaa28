"""What a 1024 x 768 viewport of an encoded image costs through itwPreviewBlocks against what the library offered before it: itwDecodeImage of
the whole image (with nothing after it -- no crop, no channel selection, no tone: a lower bound of the old way).

Streams: bc1, bc7 `basic` and bc6h `fast` encodings of the bench surface (surfaces.ldr_smooth / hdr_smooth) at 4096^2; the 16384^2 stream is that
stream tiled 4 x 4 in block space, so the waves see the same mode mix.  Legs, alternating call by call in one job:
  (a) decode_image      itwDecodeImage of the whole image into a device buffer, device-resident
  (b) preview z=...     itwPreviewBlocks, device-resident, at zoom 0.25, 1 and 2 from an interior offset (the kernel's tile route) and at
                        W / 1024, the "fit" view from offset 0 (the per-pixel route)
  (c) the same four from a host stream into a host viewport, against host_decode_image: itwDecodeImage from a host stream into a host image
      (upload + decode + download)
Timing: a host clock around one call + synchronise; per leg the median of `calls` (35) calls and their p10 / p90; `runs` (2) runs, one row each.
Required, and judged here (exit status 1 otherwise): (b) below (a) by medians on every row; (c) below host_decode_image for zoom <= 2, where only
part of the stream is uploaded.  The fit view from host memory uploads every block row: reported, not required.
One JSON object per line (stdout, and appended to profiles/preview_timing.jsonl unless --no-save).
Usage: python tools/preview_timing.py [--sizes=4096,16384] [--calls=35] [--runs=2] [--no-save] [--out=PATH]"""
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

FORMATS = [("bc1", None), ("bc7", "basic"), ("bc6h", "fast")]
VIEW_W, VIEW_H = 1024, 768


def _opt(name, default):
    return next((a[len(name) + 3:] for a in sys.argv if a.startswith(f"--{name}=")), default)


def main():
    import torch
    sizes = [int(s) for s in _opt("sizes", "4096,16384").split(",")]
    calls, runs = int(_opt("calls", "35")), int(_opt("runs", "2"))
    save = "--no-save" not in sys.argv
    out_path = _opt("out", os.path.join(ROOT, "profiles", "preview_timing.jsonl"))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L = itw_amd.lib()
    L.itwSetStream(torch.cuda.current_stream(dev).cuda_stream)
    rows, failed = [], []

    def measure(legs):
        for name, fn in legs.items():                            # warm-up: code objects, the thread's staging buffer at its largest
            assert fn() == 0 and fn() == 0, name
        torch.cuda.synchronize()
        times = {name: [] for name in legs}
        for _ in range(calls):
            for name, fn in legs.items():
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        q = lambda t, p: round(float(np.percentile(t, p)), 4)    # noqa: E731
        return {name: {"median_ms": q(t, 50), "p10_ms": q(t, 10), "p90_ms": q(t, 90)} for name, t in times.items()}

    for fmt, profile in FORMATS:
        key, bpb, px = itw_amd.DXGI_FORMAT[fmt], itw_amd.BYTES_PER_BLOCK[fmt], (8 if fmt == "bc6h" else 4)
        src = surfaces.hdr_smooth(4096, 4096) if fmt == "bc6h" else surfaces.ldr_smooth(4096, 4096)
        base_blocks = itw_amd.compress(fmt, torch.from_numpy(src.view(np.int16) if fmt == "bc6h" else src).to(dev), profile)
        torch.cuda.synchronize()
        for size in sizes:
            rep = size // 4096
            d_blocks = base_blocks.view(1024, 1024, bpb).repeat(rep, rep, 1).reshape(-1).contiguous()
            try:
                d_image = torch.empty((size, size, 4), dtype=torch.int16 if fmt == "bc6h" else torch.uint8, device=dev)
                h_image = np.empty((size, size, 4), dtype=np.uint16 if fmt == "bc6h" else np.uint8)
            except (RuntimeError, MemoryError) as e:
                print(json.dumps({"format": fmt, "size": size, "skipped": f"memory does not allow it: {e}"}), flush=True)
                continue
            h_blocks = d_blocks.cpu().numpy()
            d_surf = itw_amd.RgbaSurface(d_image.data_ptr(), size, size, size * px)
            h_surf = itw_amd.RgbaSurface(h_image.ctypes.data, size, size, size * px)
            d_out = torch.empty((VIEW_H, VIEW_W, 3), dtype=torch.uint8, device=dev)
            h_out = np.empty((VIEW_H, VIEW_W, 3), dtype=np.uint8)
            zooms = [("0.25", 0.25), ("1", 1.0), ("2", 2.0), ("fit", size / VIEW_W)]
            views = {}
            for name, z in zooms:
                at = (0, 0) if name == "fit" else (int(size / 2 / z) - VIEW_W // 2, int(size / 2 / z) - VIEW_H // 2)
                views[name] = itw_amd.preview_view(VIEW_W, VIEW_H, at[0], at[1], z, "rgb", 0x204060, 1.0)

            def decode_image(blocks_ptr, surf):
                return lambda: L.itwDecodeImage(key, blocks_ptr, C.byref(surf), None, None)

            def preview(blocks_ptr, out_ptr, v):
                return lambda: L.itwPreviewBlocks(key, blocks_ptr, size, size, C.byref(v), C.sizeof(v), out_ptr, 3 * VIEW_W)

            # what is timed is right: at zoom 1 the viewport is a crop of the decoded image's RGB (the 8-bit formats), from both pointer kinds
            if fmt != "bc6h":
                assert decode_image(d_blocks.data_ptr(), d_surf)() == 0 and preview(d_blocks.data_ptr(), d_out.data_ptr(), views["1"])() == 0
                assert preview(h_blocks.ctypes.data, h_out.ctypes.data, views["1"])() == 0
                torch.cuda.synchronize()
                x, y = views["1"].x_offset, views["1"].y_offset
                crop = d_image[y:y + VIEW_H, x:x + VIEW_W, :3]
                assert torch.equal(d_out, crop) and np.array_equal(h_out, crop.cpu().numpy()), (fmt, size, "the viewport is not the decoded image's crop")

            legs = {"decode_image": decode_image(d_blocks.data_ptr(), d_surf)}
            legs.update({f"preview z={n}": preview(d_blocks.data_ptr(), d_out.data_ptr(), views[n]) for n, _ in zooms})
            legs["host_decode_image"] = decode_image(h_blocks.ctypes.data, h_surf)
            legs.update({f"host_preview z={n}": preview(h_blocks.ctypes.data, h_out.ctypes.data, views[n]) for n, _ in zooms})
            for run in range(runs):
                t = measure(legs)
                a, c = t["decode_image"]["median_ms"], t["host_decode_image"]["median_ms"]
                row = {"format": fmt, "profile": profile, "size": size, "viewport": [VIEW_W, VIEW_H], "run": run, "calls": calls, "legs": t,
                       "b_over_a": {n: round(t[f"preview z={n}"]["median_ms"] / a, 4) for n, _ in zooms},
                       "c_over_old": {n: round(t[f"host_preview z={n}"]["median_ms"] / c, 4) for n, _ in zooms},
                       "timing": "host clock around one call + synchronise; median, p10, p90 of the calls; legs alternate call by call",
                       "device": itw_amd.device_info()}
                row["b_below_a"] = all(v < 1.0 for v in row["b_over_a"].values())
                row["c_below_old_up_to_zoom_2"] = all(row["c_over_old"][n] < 1.0 for n in ("0.25", "1", "2"))
                if not (row["b_below_a"] and row["c_below_old_up_to_zoom_2"]):
                    failed.append((fmt, size, run))
                print(json.dumps(row), flush=True)
                rows.append(row)
            del d_image, h_image, d_blocks, h_blocks
    if save and rows:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if failed:
        print("a row that must hold does not:", failed, file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
