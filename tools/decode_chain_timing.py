"""What decoding a whole file in one call costs (itwDecodeChain / itwDecodeImage) against a loop of itwDecodeBlocks, for bc1, bc7 and bc6h,
device-resident and from host memory.

Legs, per format and pointer kind, in ONE run, the variants alternating within each repetition:
  (a) cube    a 1024^2 cube map with mips down to 4x4 (6 x 9 = 54 images, all multiples of 4, so itwDecodeBlocks can decode it):
                blocks_loop   one itwDecodeBlocks per image, this build
                chain         one itwDecodeChain, this build
                parent_loop   the same loop through the PARENT commit's library (--parent-lib=PATH): the yardstick
  (b) single  one 4096^2 image:  blocks (itwDecodeBlocks, this build), image (itwDecodeImage), parent_blocks (the parent's itwDecodeBlocks)
The streams are this library's own encodes of the bench surface (bc7 veryfast, bc6h fast) and its 2x2-mean mips, so the waves see the
mode mix of real content.  Timing: a host clock around `inner` calls, each followed by a stream synchronise, after a warm-up of every
variant; best, median and (max - min) / min spread of `reps` repetitions.
Required, and judged here: (a) chain is faster than parent_loop (medians) for every format and pointer kind -- the tool exits 1 otherwise;
(b) image is not slower than parent_blocks by more than parent_blocks' own min-max spread (recorded as b_within_parent_spread).
Recorded, not judged: hbm_fraction of (b) device-resident = (stream + texels) bytes / median time / 8 TB/s.
Without --parent-lib the parent legs are this build's itwDecodeBlocks (whose code no later commit may change) and the row says so.
One JSON object per line (stdout, and appended to profiles/decode_chain_timing.jsonl unless --no-save).
Usage: python tools/decode_chain_timing.py [reps] [inner] [--parent-lib=PATH] [--no-save] [--out=PATH]"""
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

FORMATS = [("bc1", None), ("bc7", "veryfast"), ("bc6h", "fast")]
HBM_BYTES_PER_S = 8e12


def _source(fmt, size):
    return surfaces.hdr_smooth(size, size, seed=surfaces.SEED + 3) if fmt == "bc6h" else surfaces.ldr_smooth(size, size, seed=surfaces.SEED)


def _bind(L):
    L.itwDecodeBlocks.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    L.itwDecodeBlocks.restype = C.c_int
    L.itwSetStream.argtypes = [C.c_void_p]
    L.itwSetStream.restype = None
    return L


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    inner = int(args[1]) if len(args) > 1 else 5
    save = "--no-save" not in sys.argv
    out_path = next((a[6:] for a in sys.argv if a.startswith("--out=")), os.path.join(ROOT, "profiles", "decode_chain_timing.jsonl"))
    parent_path = next((a[13:] for a in sys.argv if a.startswith("--parent-lib=")), None)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L = itw_amd.lib()
    P = _bind(C.CDLL(parent_path)) if parent_path else L
    stream = torch.cuda.current_stream(dev).cuda_stream
    L.itwSetStream(stream)
    P.itwSetStream(stream)
    parent_note = os.path.basename(parent_path) + " built from the parent commit" if parent_path else "not given: this build's unchanged itwDecodeBlocks"

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / inner

    def run(variants):
        for fn in variants.values():                             # warm-up: code objects, the chain call's buffer at its largest
            fn(); fn()
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(reps):
            for name, fn in variants.items():
                times[name].append(timed(fn))
        out = {}
        for name, t in times.items():
            t = sorted(t)
            out[name] = {"ms": round(t[0], 4), "median_ms": round(t[len(t) // 2], 4), "max_ms": round(t[-1], 4), "spread": round((t[-1] - t[0]) / t[0], 3)}
        return out

    rows, failed = [], []
    for fmt, profile in FORMATS:
        key = itw_amd.DXGI_FORMAT[fmt]
        px, bpb = (8 if fmt == "bc6h" else 4), itw_amd.BYTES_PER_BLOCK[fmt]
        tdtype = torch.int16 if fmt == "bc6h" else torch.uint8
        ndtype = np.uint16 if fmt == "bc6h" else np.uint8

        # the streams: a face's chain 1024 .. 4, six times; one 4096^2 image
        levels = [lv for lv in itw_amd.mip_chain(_source(fmt, 1024)) if lv.shape[0] >= 4]
        face = [torch.from_numpy(lv.view(np.int16) if fmt == "bc6h" else lv).to(dev) for lv in levels]
        ok, cube_blocks = itw_amd.compress_chain(fmt, face * 6, profile=profile)
        assert ok
        big = _source(fmt, 4096)
        big_blocks = itw_amd.compress(fmt, torch.from_numpy(big.view(np.int16) if fmt == "bc6h" else big).to(dev), profile)
        torch.cuda.synchronize()
        sizes = [tuple(lv.shape[:2]) for lv in levels] * 6
        assert len(sizes) == 54
        offs = np.concatenate([[0], np.cumsum([(h // 4) * (w // 4) * bpb for h, w in sizes])]).tolist()

        for kind in ("device", "host"):
            if kind == "device":
                blocks, single = cube_blocks, big_blocks
                outs = [torch.empty((h, w, 4), dtype=tdtype, device=dev) for h, w in sizes]
                one = torch.empty((4096, 4096, 4), dtype=tdtype, device=dev)
                ptr = lambda t: t.data_ptr()                     # noqa: E731
            else:
                blocks, single = cube_blocks.cpu().numpy(), big_blocks.cpu().numpy()
                outs = [np.empty((h, w, 4), dtype=ndtype) for h, w in sizes]
                one = np.empty((4096, 4096, 4), dtype=ndtype)
                ptr = lambda a: a.ctypes.data                    # noqa: E731
            surfs = (itw_amd.RgbaSurface * 54)(*[itw_amd.RgbaSurface(ptr(o), w, h, w * px) for o, (h, w) in zip(outs, sizes)])
            one_surf = itw_amd.RgbaSurface(ptr(one), 4096, 4096, 4096 * px)
            bp, sp, optrs = ptr(blocks), ptr(single), [ptr(o) for o in outs]

            def loop(lib):
                def fn():
                    for i, (h, w) in enumerate(sizes):
                        assert lib.itwDecodeBlocks(key, bp + offs[i], w, h, optrs[i], w * px, None) == 0
                return fn

            def chain():
                assert L.itwDecodeChain(key, bp, C.cast(surfs, C.c_void_p), 54, None, None) == 0

            def blocks_of(lib):
                return lambda: lib.itwDecodeBlocks(key, sp, 4096, 4096, ptr(one), 4096 * px, None)

            def image():
                assert L.itwDecodeImage(key, sp, C.byref(one_surf), None, None) == 0

            # what the legs time is one decode: the chain call writes what the loop writes
            loop(L)()
            torch.cuda.synchronize()
            want = [o.clone() if kind == "device" else o.copy() for o in outs]
            for o in outs:
                o.zero_() if kind == "device" else o.fill(0)
            chain()
            torch.cuda.synchronize()
            same = all((torch.equal(a, b) if kind == "device" else np.array_equal(a, b)) for a, b in zip(outs, want))
            assert same, (fmt, kind, "itwDecodeChain and the itwDecodeBlocks loop disagree")

            a = run({"blocks_loop": loop(L), "chain": chain, "parent_loop": loop(P)})
            b = run({"blocks": blocks_of(L), "image": image, "parent_blocks": blocks_of(P)})
            base = {"format": fmt, "pointers": kind, "reps": reps, "inner": inner, "parent": parent_note,
                    "timing": "host clock around calls that each end in a stream synchronise", "device": itw_amd.device_info()}
            ra = dict(base, leg="a_cube_1024_mips_to_4", images=54, blocks=offs[-1] // bpb, variants=a,
                      chain_vs_parent_loop=round(a["chain"]["median_ms"] / a["parent_loop"]["median_ms"], 4),
                      a_faster_than_parent=a["chain"]["median_ms"] < a["parent_loop"]["median_ms"])
            pb = b["parent_blocks"]
            rb = dict(base, leg="b_single_4096", images=1, blocks=1024 * 1024, variants=b,
                      image_vs_parent_blocks=round(b["image"]["median_ms"] / pb["median_ms"], 4),
                      b_within_parent_spread=b["image"]["median_ms"] - pb["median_ms"] <= pb["max_ms"] - pb["ms"])
            if kind == "device":
                rb["hbm_fraction"] = round((1024 * 1024 * bpb + 4096 * 4096 * px) / (b["image"]["median_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
            for r in (ra, rb):
                print(json.dumps(r), flush=True)
                rows.append(r)
            if not ra["a_faster_than_parent"]:
                failed.append((fmt, kind))
    if save and rows:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if failed:
        print("leg (a): itwDecodeChain is NOT faster than the parent's itwDecodeBlocks loop for", failed, file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
