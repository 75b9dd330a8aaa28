"""The battery one child process of tests/test_gpu_launch_switches.py runs: every BC7 call below through the hooks build
(itw_amd.test_lib()), the route witness (itwTestBc7RouteCounters) reset before and read after each call.  The switches under test are read
once per process, so they come from this process's environment -- ITW_BC7_PATH among them: nothing here calls itwSetBc7Path.  The script
writes every output stream and every counter vector to an .npz and asserts nothing; the parent compares.

    python tests/_launch_switch_child.py INPUTS.npz OUTPUTS.npz [--product] [--host-runs CUTS]

INPUTS.npz holds the images the cases name (A_rgb, A_rgba, B_rgb, B_rgba, host_photo); OUTPUTS.npz gets `<case>.bytes` and `<case>.ctr` per
case, in the order of device_cases() + host_cases().  --product: the device-resident part once more through the product library
(`product:<case>.bytes`, no counters).
"""
import argparse
import contextlib
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# A: 129 x 65 = 8 385 blocks = 33 chunks of 256, one above two_bands' 32, a ragged last stripe and a partial last chunk.  B: 561 blocks, one band.
SHAPES = {"A": (516, 260), "B": (132, 68)}                # width x height in texels
HOST_SHAPE = (64, 256)                                    # 16 x 64 blocks: the least ITW_HOST_RUNS cuts
# The cut of tests/test_gpu_host_runs_small.py is "0.125,0.625": a first run of 8 block rows = 128 blocks.  bc7_pilot_estimate looks at chunks
# 8 i + 3 of a run (csrc/bc7.hip sel_chunk), and a run of 128 blocks has no chunk 3 (blocks 768 ..): the estimate samples nothing, read_verdict
# (csrc/abi.hip) leaves the thread's verdict alone and no ITW_STAGED_VERDICT_THR can send a run wide.  The least first run that samples a
# block is 49 block rows = 784 blocks (16 of them in chunk 3); the other two runs keep a few rows each.
HOST_RUNS = "0.765625,0.890625"                           # block rows [0, 49) [49, 57) [57, 64)
HOST_PROFILES = ("slow", "alpha_slow", "basic")
HOST_CALLS = 4
SETTINGS = ("slow", "alpha_slow", "basic", "alpha_basic", "alpha_slow_ranked7")
PILOTS = (100, 0)
KNOBS = {"unset": None, "pairs0": ("ITW_BC7_PAIRS", "0"), "paircap1": ("ITW_BC7_PAIR_CAP", "1"), "rot0": ("ITW_BC7_ROT_TASKS", "0")}


def is_rgba(settings):
    return settings.startswith("alpha")


def profile_of(settings):
    """the GetProfile_* a settings name starts from; `alpha_slow_ranked7` is alpha_slow with fastSkipTreshold_mode7 = 3 -- the one struct
    that reaches launch_alpha_first with a bound"""
    return "alpha_slow" if settings == "alpha_slow_ranked7" else settings


def device_cases():
    """(case name, image key, settings, pilot percent or None, per-call knob): `slow` on A under both pilot settings x the four per-call knobs,
    every other struct once on A and B, and `slow` on a view of A that no 16-byte access fits"""
    out = []
    for shape in SHAPES:
        for st in SETTINGS:
            img = f"{shape}_{'rgba' if is_rgba(st) else 'rgb'}"
            if shape == "A" and st == "slow":
                out += [(f"A/slow/pilot{p}/{k}", img, st, p, k) for p in PILOTS for k in KNOBS]
            else:
                out.append((f"{shape}/{st}", img, st, None, "unset"))
    out.append(("A_unaligned/slow", "A_rgb", "slow", None, "unset"))
    return out


def host_cases():
    """(case name, settings, device destination): four calls per profile on the photograph, then one `slow` call into device memory"""
    out = [(f"host/{p}/call{k + 1}", p, False) for p in HOST_PROFILES for k in range(HOST_CALLS)]
    out.append(("host/slow/device_dst", "slow", True))
    return out


@contextlib.contextmanager
def knob(pair):
    if pair:
        os.environ[pair[0]] = pair[1]
    try:
        yield
    finally:
        if pair:
            del os.environ[pair[0]]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("inputs")
    ap.add_argument("outputs")
    ap.add_argument("--product", action="store_true", help="also run the device-resident part through the product library")
    ap.add_argument("--host-runs", default=HOST_RUNS, help="ITW_HOST_RUNS around the host-pointer calls")
    args = ap.parse_args(argv)

    for p in (ROOT, os.path.join(ROOT, "intel-texture-works-plugin_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import itw_amd

    images = dict(np.load(args.inputs))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    T = itw_amd.test_lib()
    names = itw_amd.BC7_ROUTE_COUNTERS
    out = {}

    def settings_of(L, name):
        s = itw_amd.Bc7Settings()
        getattr(L, "GetProfile_" + profile_of(name))(C.byref(s))
        if name == "alpha_slow_ranked7":
            s.fastSkipTreshold_mode7 = 3
        return s

    def counted(case, call):
        """`call` between a reset and a read of the route witness"""
        T.itwTestBc7RouteCountersReset()
        call()
        torch.cuda.synchronize()
        buf = (C.c_int64 * len(names))()
        T.itwTestBc7RouteCounters(buf, len(names))
        out[case + ".ctr"] = np.array(list(buf), np.int64)

    def resident(L, img, st, unaligned=False):
        """one device-resident CompressBlocksBC7; `unaligned`: from a view 12 bytes past a 16-byte boundary whose pitch is no multiple of 16"""
        h, w = img.shape[:2]
        if unaligned:
            pitch = w * 4 + 20
            store = torch.zeros(h * pitch + 32, dtype=torch.uint8, device=dev)
            off = (12 - store.data_ptr()) % 16
            rows = store[off:off + h * pitch].view(h, pitch)
            rows[:, :w * 4] = torch.from_numpy(img.reshape(h, w * 4)).to(dev)
            ptr = store.data_ptr() + off
            assert ptr % 16 == 12 and pitch % 16 != 0
        else:
            store = torch.from_numpy(img).to(dev)
            ptr, pitch = store.data_ptr(), w * 4
        dst = torch.zeros((h // 4) * (w // 4) * 16, dtype=torch.uint8, device=dev)
        surf = itw_amd.RgbaSurface(ptr, w, h, pitch)
        torch.cuda.synchronize()
        L.CompressBlocksBC7(C.byref(surf), C.c_void_p(dst.data_ptr()), C.byref(st))
        torch.cuda.synchronize()
        return dst.cpu().numpy()

    def device_part(L, prefix, count):
        for case, key, st_name, pilot, k in device_cases():
            st = settings_of(L, st_name)
            L.itwSetBc7Pilot(-2 if pilot is None else pilot)
            with knob(KNOBS[k]):
                def call():
                    out[prefix + case + ".bytes"] = resident(L, images[key], st, unaligned=case.startswith("A_unaligned"))
                if count:
                    counted(case, call)
                else:
                    call()
        L.itwSetBc7Pilot(-2)

    device_part(T, "", True)

    photo = images["host_photo"]
    h, w = photo.shape[:2]
    nbytes = (h // 4) * (w // 4) * 16
    for case, st_name, dst_dev in host_cases():
        st = settings_of(T, st_name)
        surf = itw_amd.RgbaSurface(photo.ctypes.data, w, h, photo.strides[0])
        dst = torch.zeros(nbytes, dtype=torch.uint8, device=dev) if dst_dev else np.zeros(nbytes, np.uint8)
        dst_ptr = dst.data_ptr() if dst_dev else dst.ctypes.data
        with knob(("ITW_HOST_RUNS", args.host_runs)):
            counted(case, lambda: T.CompressBlocksBC7(C.byref(surf), C.c_void_p(dst_ptr), C.byref(st)))
        out[case + ".bytes"] = dst.cpu().numpy() if dst_dev else dst

    if args.product:
        device_part(itw_amd.lib(), "product:", False)

    np.savez(args.outputs, **out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
