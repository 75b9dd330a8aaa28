"""What decoding costs through the three entry points (itwDecodeChain, itwDecodeImage, itwDecodeBlocks) against the PARENT commit's
itwDecodeBlocks, device-resident and from host memory.  All three run one kernel (csrc/decode_chain.hip); the parent's library, built from
the commit before, is the yardstick and is always needed: --parent-lib=PATH.

Legs, per format and pointer kind, in ONE run, the variants alternating within each repetition:
  (a) cube    bc1, bc7, bc6h: a 1024^2 cube map with mips down to 4x4 (6 x 9 = 54 images, all multiples of 4, so itwDecodeBlocks can decode it):
                blocks_loop   one itwDecodeBlocks per image, this build
                chain         one itwDecodeChain, this build
                parent_loop   the same loop through the parent's library
  (b) single  every format (bc1, bc3, bc4, bc5, bc4_snorm, bc5_snorm, bc7, bc6h), one 4096^2 image:
                blocks (itwDecodeBlocks, this build), image (itwDecodeImage), parent_blocks (the parent's itwDecodeBlocks)
The streams are this library's own encodes of the bench surface (bc7 veryfast, bc6h fast; a normal map for the SNORM pair) and its
2x2-mean mips, so the waves see the mode mix of real content.  Timing: a host clock around `inner` calls, each followed by a stream
synchronise, after a warm-up of every variant; best, median and (max - min) / min spread of `reps` repetitions.
Required, and judged here: (a) chain is faster than parent_loop (medians) for every format and pointer kind -- the tool exits 1 otherwise.
Recorded for the reader to judge: (b) neither blocks nor image is slower than parent_blocks, by medians, by more than parent_blocks' own
min-max spread (blocks_within_parent_spread, b_within_parent_spread); hbm_fraction of (b) device-resident = (stream + texels) bytes /
median time / 8 TB/s.
One JSON object per line (stdout, and appended to profiles/decode_chain_timing.jsonl unless --no-save).
--bc6hs: the signed reading of BC6H (ITW_FORMAT_BC6H_SIGNED) next to the unsigned one, this build only (the parent does not know the code, so
no --parent-lib): the same bc6h streams read under 95 and under 0x8E8E, the legs alternating in one run -- (s) one 4096^2 itwDecodeBlocks,
(c) the 54-image cube through one itwDecodeChain and through the itwDecodeBlocks loop -- device-resident and from host memory; per row
signed_vs_unsigned by medians with each leg's spread beside it.  Appended to profiles/bc6hs_timing.jsonl.
Usage: python tools/decode_chain_timing.py --parent-lib=PATH [reps] [inner] [--no-save] [--out=PATH]
       python tools/decode_chain_timing.py --bc6hs [reps] [inner] [--no-save] [--out=PATH]"""
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

FORMATS = [("bc1", None, True), ("bc7", "veryfast", True), ("bc6h", "fast", True),                  # (format, profile, has a cube leg)
           ("bc3", None, False), ("bc4", None, False), ("bc5", None, False), ("bc4_snorm", None, False), ("bc5_snorm", None, False)]
HBM_BYTES_PER_S = 8e12


_sources = {}


def _source(fmt, size):
    gen = surfaces.hdr_smooth if fmt == "bc6h" else surfaces.snorm_normal_map if fmt in itw_amd.SIGNED_FORMATS else surfaces.ldr_smooth
    if (gen, size) not in _sources:
        _sources[(gen, size)] = gen(size, size)
    return _sources[(gen, size)]


def _bind(L):
    L.itwDecodeBlocks.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    L.itwDecodeBlocks.restype = C.c_int
    L.itwSetStream.argtypes = [C.c_void_p]
    L.itwSetStream.restype = None
    return L


def bc6hs_legs(torch, dev, L, run, reps, inner):
    """The --bc6hs rows: one bc6h stream (this library's `fast` encode of the bench surface: valid blocks under either reading) decoded under 95
    and under ITW_FORMAT_BC6H_SIGNED, alternating."""
    U, S = itw_amd.DXGI_FORMAT["bc6h"], itw_amd.DXGI_FORMAT["bc6h_signed"]
    levels = [lv for lv in itw_amd.mip_chain(_source("bc6h", 1024)) if lv.shape[0] >= 4]
    ok, cube_blocks = itw_amd.compress_chain("bc6h", [torch.from_numpy(lv.view(np.int16)).to(dev) for lv in levels] * 6, profile="fast")
    assert ok
    sizes = [tuple(lv.shape[:2]) for lv in levels] * 6
    offs = np.concatenate([[0], np.cumsum([(h // 4) * (w // 4) * 16 for h, w in sizes])]).tolist()
    big_blocks = itw_amd.compress("bc6h", torch.from_numpy(_source("bc6h", 4096).view(np.int16)).to(dev), "fast")
    torch.cuda.synchronize()
    rows = []
    for kind in ("device", "host"):
        if kind == "device":
            blocks, single = cube_blocks, big_blocks
            outs = [torch.empty((h, w, 4), dtype=torch.int16, device=dev) for h, w in sizes]
            one = torch.empty((4096, 4096, 4), dtype=torch.int16, device=dev)
            ptr = lambda t: t.data_ptr()                         # noqa: E731
        else:
            blocks, single = cube_blocks.cpu().numpy(), big_blocks.cpu().numpy()
            outs = [np.empty((h, w, 4), dtype=np.uint16) for h, w in sizes]
            one = np.empty((4096, 4096, 4), dtype=np.uint16)
            ptr = lambda a: a.ctypes.data                        # noqa: E731
        surfs = (itw_amd.RgbaSurface * len(sizes))(*[itw_amd.RgbaSurface(ptr(o), w, h, w * 8) for o, (h, w) in zip(outs, sizes)])
        bp, sp, optrs = ptr(blocks), ptr(single), [ptr(o) for o in outs]

        def loop(key):
            def fn():
                for i, (h, w) in enumerate(sizes):
                    assert L.itwDecodeBlocks(key, bp + offs[i], w, h, optrs[i], w * 8, None) == 0
            return fn

        def chain(key):
            return lambda: L.itwDecodeChain(key, bp, C.cast(surfs, C.c_void_p), 54, None, None)

        def blocks_of(key):
            return lambda: L.itwDecodeBlocks(key, sp, 4096, 4096, ptr(one), 4096 * 8, None)

        assert chain(S)() == 0 and blocks_of(S)() == 0
        base = {"format": "bc6h_signed beside bc6h", "pointers": kind, "reps": reps, "inner": inner,
                "timing": "host clock around calls that each end in a stream synchronise", "device": itw_amd.device_info()}
        s = run({"unsigned_blocks": blocks_of(U), "signed_blocks": blocks_of(S)})
        row = dict(base, leg="s_single_4096", images=1, blocks=1024 * 1024, variants=s,
                   signed_vs_unsigned=round(s["signed_blocks"]["median_ms"] / s["unsigned_blocks"]["median_ms"], 4))
        if kind == "device":
            row["hbm_fraction_signed"] = round((1024 * 1024 * 16 + 4096 * 4096 * 8) / (s["signed_blocks"]["median_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
        c = run({"unsigned_chain": chain(U), "signed_chain": chain(S), "unsigned_loop": loop(U), "signed_loop": loop(S)})
        rows += [row, dict(base, leg="c_cube_1024_mips_to_4", images=54, blocks=offs[-1] // 16, variants=c,
                           signed_vs_unsigned_chain=round(c["signed_chain"]["median_ms"] / c["unsigned_chain"]["median_ms"], 4),
                           signed_chain_vs_signed_loop=round(c["signed_chain"]["median_ms"] / c["signed_loop"]["median_ms"], 4))]
        for r in rows[-2:]:
            print(json.dumps(r), flush=True)
    return rows


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    inner = int(args[1]) if len(args) > 1 else 5
    save = "--no-save" not in sys.argv
    signed_legs = "--bc6hs" in sys.argv
    out_path = next((a[6:] for a in sys.argv if a.startswith("--out=")),
                    os.path.join(ROOT, "profiles", "bc6hs_timing.jsonl" if signed_legs else "decode_chain_timing.jsonl"))
    parent_path = next((a[13:] for a in sys.argv if a.startswith("--parent-lib=")), None)
    if not parent_path and not signed_legs:
        sys.exit("--parent-lib=PATH is required: the parent commit's libispc_texcomp.so is what every leg is measured against")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L = itw_amd.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    L.itwSetStream(stream)
    if not signed_legs:
        P = _bind(C.CDLL(parent_path))
        P.itwSetStream(stream)
        parent_note = os.path.basename(parent_path) + " built from the parent commit"

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
    if signed_legs:
        rows = bc6hs_legs(torch, dev, L, run, reps, inner)
        if save and rows:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "a") as f:
                for r in rows:
                    f.write(json.dumps(r) + "\n")
        return
    for fmt, profile, cube in FORMATS:
        key = itw_amd.DXGI_FORMAT[fmt]
        px, bpb = (8 if fmt == "bc6h" else 4), itw_amd.BYTES_PER_BLOCK[fmt]
        signed = fmt in itw_amd.SIGNED_FORMATS
        tdtype = torch.int16 if fmt == "bc6h" else torch.int8 if signed else torch.uint8
        ndtype = np.uint16 if fmt == "bc6h" else np.int8 if signed else np.uint8

        # the streams: a face's chain 1024 .. 4, six times; one 4096^2 image
        sizes, offs, cube_blocks = [], [0], None
        if cube:
            levels = [lv for lv in itw_amd.mip_chain(_source(fmt, 1024)) if lv.shape[0] >= 4]
            face = [torch.from_numpy(lv.view(np.int16) if fmt == "bc6h" else lv).to(dev) for lv in levels]
            ok, cube_blocks = itw_amd.compress_chain(fmt, face * 6, profile=profile)
            assert ok
            sizes = [tuple(lv.shape[:2]) for lv in levels] * 6
            assert len(sizes) == 54
            offs = np.concatenate([[0], np.cumsum([(h // 4) * (w // 4) * bpb for h, w in sizes])]).tolist()
        big = _source(fmt, 4096)
        big_blocks = itw_amd.compress(fmt, torch.from_numpy(big.view(np.int16) if fmt == "bc6h" else big).to(dev), profile)
        torch.cuda.synchronize()

        for kind in ("device", "host"):
            if kind == "device":
                blocks, single = cube_blocks if cube else big_blocks, big_blocks
                outs = [torch.empty((h, w, 4), dtype=tdtype, device=dev) for h, w in sizes]
                one = torch.empty((4096, 4096, 4), dtype=tdtype, device=dev)
                ptr = lambda t: t.data_ptr()                     # noqa: E731
            else:
                blocks, single = (cube_blocks if cube else big_blocks).cpu().numpy(), big_blocks.cpu().numpy()
                outs = [np.empty((h, w, 4), dtype=ndtype) for h, w in sizes]
                one = np.empty((4096, 4096, 4), dtype=ndtype)
                ptr = lambda a: a.ctypes.data                    # noqa: E731
            surfs = (itw_amd.RgbaSurface * len(sizes))(*[itw_amd.RgbaSurface(ptr(o), w, h, w * px) for o, (h, w) in zip(outs, sizes)])
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

            base = {"format": fmt, "pointers": kind, "reps": reps, "inner": inner, "parent": parent_note,
                    "timing": "host clock around calls that each end in a stream synchronise", "device": itw_amd.device_info()}
            found = []
            if cube:
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
                ra = dict(base, leg="a_cube_1024_mips_to_4", images=54, blocks=offs[-1] // bpb, variants=a,
                          chain_vs_parent_loop=round(a["chain"]["median_ms"] / a["parent_loop"]["median_ms"], 4),
                          a_faster_than_parent=a["chain"]["median_ms"] < a["parent_loop"]["median_ms"])
                found.append(ra)
                if not ra["a_faster_than_parent"]:
                    failed.append((fmt, kind))
            # ... and this build's itwDecodeBlocks writes what the parent's writes
            blocks_of(P)()
            torch.cuda.synchronize()
            want_one = one.clone() if kind == "device" else one.copy()
            one.zero_() if kind == "device" else one.fill(0)
            blocks_of(L)()
            torch.cuda.synchronize()
            assert torch.equal(one, want_one) if kind == "device" else np.array_equal(one, want_one), (fmt, kind, "itwDecodeBlocks differs from the parent's")

            b = run({"blocks": blocks_of(L), "image": image, "parent_blocks": blocks_of(P)})
            pb = b["parent_blocks"]
            rb = dict(base, leg="b_single_4096", images=1, blocks=1024 * 1024, variants=b,
                      blocks_vs_parent_blocks=round(b["blocks"]["median_ms"] / pb["median_ms"], 4),
                      blocks_within_parent_spread=b["blocks"]["median_ms"] - pb["median_ms"] <= pb["max_ms"] - pb["ms"],
                      image_vs_parent_blocks=round(b["image"]["median_ms"] / pb["median_ms"], 4),
                      b_within_parent_spread=b["image"]["median_ms"] - pb["median_ms"] <= pb["max_ms"] - pb["ms"])
            if kind == "device":
                rb["hbm_fraction"] = round((1024 * 1024 * bpb + 4096 * 4096 * px) / (b["image"]["median_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
            for r in found + [rb]:
                print(json.dumps(r), flush=True)
                rows.append(r)
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
