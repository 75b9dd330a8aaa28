"""One run of the encode host layer's timing rows against the build under ROOT (a checkout with its libraries built): the slice loop at 4096^2
with 64 slices from pageable host memory and a progress callback (BC7 `basic` / `slow`, BC6H `slow`, BC1, ETC1 `slow`), the 1024^2 BC7 `basic`
cube-map chain and the 2048^2 2D chain (device-resident and from host memory), and BC6H `slow` 4096^2 as one host-pointer call.  Then the
routes of compress() itself, each as one CompressBlocks* call at 4096^2 from pageable host memory -- BC7 `slow` on the smooth surface (windows
with the verdict), on a tiled photograph (staged runs that go wide, with the probe) and, in a child process with ITW_HOST_WINDOWS_OFF=1, on
the smooth surface again (staged runs as bands); BC6H `fast` (four runs); BC1 (a single run) -- and the small-call path: 3000 64 x 64 BC1 and
BC7 `basic` host-pointer calls from one thread, the median per call.  Per row the
median and best of N calls and the first 16 hex digits of the output's SHA-256, one JSON object per line (stdout, and appended to OUT_JSONL).
Two builds are compared by running this file once per build and run, alternating (profiles/host_layer_refactor_timing.jsonl,
profiles/host_route_refactor_timing.jsonl).
Usage: python tools/host_layer_timing.py ROOT BUILD_TAG RUN_INDEX OUT_JSONL [calls=35]"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT, TAG, RUN, OUT = os.path.abspath(sys.argv[1]), sys.argv[2], int(sys.argv[3]), sys.argv[4]
CALLS = int(sys.argv[5]) if len(sys.argv) > 5 else 35
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))
import numpy as np                      # noqa: E402
import torch                            # noqa: E402
import itw_amd                          # noqa: E402
from itw_amd import surfaces            # noqa: E402

assert os.path.abspath(itw_amd.lib_path()).startswith(ROOT), itw_amd.lib_path()
CACHE = os.path.join(tempfile.gettempdir(), "itw_timing_cache")      # the generated surfaces, shared by the runs of a job
os.makedirs(CACHE, exist_ok=True)


def cached(name, make):
    p = os.path.join(CACHE, name + ".npy")
    if os.path.exists(p):
        return np.load(p)
    a = np.ascontiguousarray(make())
    np.save(p, a)
    return a


def median_ms(fn, sync=lambda: None):
    fn(); sync(); fn(); sync()
    ts = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        fn(); sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


rows = []


def emit(row, med, best, out):
    data = out.cpu().numpy() if hasattr(out, "cpu") else out
    rows.append({"build": TAG, "run": RUN, "row": row, "median_ms": round(med, 4), "best_ms": round(best, 4), "calls": CALLS,
                 "sha256_16": hashlib.sha256(data.tobytes()).hexdigest()[:16]})
    print(json.dumps(rows[-1]), flush=True)


def main():
    L = itw_amd.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ldr = cached("ldr4096", lambda: surfaces.ldr_smooth(4096, 4096))
    hdr = cached("hdr4096", lambda: surfaces.hdr_smooth(4096, 4096))
    # sliced@64 at 4096^2, pageable host memory, a progress callback installed
    for fmt, prof in (("bc7", "basic"), ("bc7", "slow"), ("bc6h", "slow"), ("bc1", None), ("etc1", "slow")):
        img = hdr if fmt == "bc6h" else ldr
        out = np.zeros(itw_amd.block_count(fmt, 4096, 4096) * itw_amd.BYTES_PER_BLOCK[fmt], np.uint8)
        n = [0]

        def cb(i, t, u):
            n[0] += 1
            return True
        med, best = median_ms(lambda: itw_amd.compress_image(fmt, img, prof, multithreaded=False, progress=cb, out=out))
        assert n[0] == 63 * (CALLS + 2), n[0]
        emit(f"sliced@64 4096^2 host {fmt} {prof or '-'}", med, best, out)
    # chains: the 1024^2 BC7 `basic` cube map and the 2048^2 2D chain, device-resident and from host memory
    st = itw_amd.bc7_profile("basic")
    sp = C.cast(C.byref(st), C.c_void_p)
    for name, size, faces in (("cube 1024^2", 1024, 6), ("2d 2048^2", 2048, 1)):
        images = []
        for f in range(faces):
            top = cached(f"ldr{size}_{f}", lambda: surfaces.ldr_smooth(size, size, seed=100 + f))
            images += [np.ascontiguousarray(lv) for lv in itw_amd.mip_chain(top)]
        nbytes = itw_amd.chain_bytes("bc7", images)
        for where in ("device", "host"):
            if where == "host":
                srcs, out = images, np.zeros(nbytes, np.uint8)
                arr = (itw_amd.RgbaSurface * len(srcs))(*[itw_amd.RgbaSurface(a.ctypes.data, a.shape[1], a.shape[0], a.strides[0]) for a in srcs])
                dst = out.ctypes.data
            else:
                srcs, out = [torch.from_numpy(a).to(dev) for a in images], torch.zeros(nbytes, dtype=torch.uint8, device=dev)
                arr = (itw_amd.RgbaSurface * len(srcs))(*[itw_amd.RgbaSurface(t.data_ptr(), t.shape[1], t.shape[0], t.stride(0)) for t in srcs])
                dst = out.data_ptr()
                L.itwSetStream(torch.cuda.current_stream(dev).cuda_stream)
                torch.cuda.synchronize()

            def chain():
                assert L.itwCompressImageChainEx(C.cast(arr, C.c_void_p), len(srcs), dst, 98, sp, None, None)
            med, best = median_ms(chain, torch.cuda.synchronize)
            emit(f"chain bc7 basic {name} {where}", med, best, out)
    # BC6H `slow` 4096^2 as one host-pointer call
    s6 = itw_amd.bc6h_profile("slow")
    surf = itw_amd.RgbaSurface(hdr.ctypes.data, 4096, 4096, hdr.strides[0])
    out = np.zeros(1024 * 1024 * 16, np.uint8)
    med, best = median_ms(lambda: L.CompressBlocksBC6H(C.byref(surf), out.ctypes.data, C.byref(s6)))
    emit("one call 4096^2 host bc6h slow", med, best, out)
    one_call_rows(L, ldr, hdr)
    small_call_rows(L)
    write_rows()
    # ITW_HOST_WINDOWS_OFF is a property of the process: its row comes from a child of this file
    subprocess.run([sys.executable, os.path.abspath(__file__), ROOT, TAG, str(RUN), OUT, str(CALLS)], check=True,
                   env=dict(os.environ, ITW_HOST_WINDOWS_OFF="1"))


def write_rows():
    with open(OUT, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


def one_call(L, fmt, img, prof):
    """One CompressBlocks* call over a 4096^2 surface in pageable host memory: compress()'s own routes"""
    st = itw_amd.bc7_profile(prof) if fmt == "bc7" else itw_amd.bc6h_profile(prof) if fmt == "bc6h" else None
    fn = {"bc7": L.CompressBlocksBC7, "bc6h": L.CompressBlocksBC6H, "bc1": L.CompressBlocksBC1}[fmt]
    surf = itw_amd.RgbaSurface(img.ctypes.data, img.shape[1], img.shape[0], img.strides[0])
    out = np.zeros(itw_amd.block_count(fmt, img.shape[1], img.shape[0]) * itw_amd.BYTES_PER_BLOCK[fmt], np.uint8)
    args = (C.byref(surf), out.ctypes.data) + ((C.byref(st),) if st is not None else ())
    med, best = median_ms(lambda: fn(*args))
    return med, best, out


def photograph():
    bab = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "inputs.npz"))["baboon"]
    return np.tile(bab, (4096 // bab.shape[0], 4096 // bab.shape[1], 1))


def one_call_rows(L, ldr, hdr):
    # windows whose first leaves the verdict; staged runs that go wide, with the probe (the photograph's verdict holds from the second call on);
    # four runs without bands; one run
    emit("one call 4096^2 host bc7 slow smooth (windows + verdict)", *one_call(L, "bc7", ldr, "slow"))
    emit("one call 4096^2 host bc7 slow photograph (wide runs + probe)", *one_call(L, "bc7", cached("baboon4096", photograph), "slow"))
    emit("one call 4096^2 host bc6h fast (four runs)", *one_call(L, "bc6h", hdr, "fast"))
    emit("one call 4096^2 host bc1 (single run)", *one_call(L, "bc1", ldr, None))


def small_call_rows(L, n=3000):
    """The small-call path: 64 x 64 host-pointer calls from one thread, the median per call"""
    img = np.ascontiguousarray(surfaces.ldr_smooth(64, 64))
    surf = itw_amd.RgbaSurface(img.ctypes.data, 64, 64, img.strides[0])
    st = itw_amd.bc7_profile("basic")
    for name, call, nbytes in (("bc1", lambda o: L.CompressBlocksBC1(C.byref(surf), o), 2048),
                               ("bc7 basic", lambda o: L.CompressBlocksBC7(C.byref(surf), o, C.byref(st)), 4096)):
        out = np.zeros(nbytes, np.uint8)
        for _ in range(50):
            call(out.ctypes.data)
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            call(out.ctypes.data)
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        rows.append({"build": TAG, "run": RUN, "row": f"small calls 64x64 host {name}", "median_ms": round(ts[n // 2], 5), "best_ms": round(ts[0], 5),
                     "calls": n, "sha256_16": hashlib.sha256(out.tobytes()).hexdigest()[:16]})
        print(json.dumps(rows[-1]), flush=True)


def windows_off_row():
    L = itw_amd.lib()
    torch.cuda.set_device(torch.device("cuda:0"))
    ldr = cached("ldr4096", lambda: surfaces.ldr_smooth(4096, 4096))
    emit("one call 4096^2 host bc7 slow smooth, ITW_HOST_WINDOWS_OFF=1 (runs as bands)", *one_call(L, "bc7", ldr, "slow"))
    write_rows()


if os.environ.get("ITW_HOST_WINDOWS_OFF"):
    windows_off_row()
else:
    main()
