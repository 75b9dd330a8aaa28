"""The surfaces and launch switches of tests/test_gpu_bc7_bound_kernel.py and what a build's RGB bounded order counts on them (GPU).

    python tools/bc7_bound_kernel_counters.py OUT.json

encodes every case below with BC7 `slow` through the HOOKS library of the tree it is run from, deep path, and writes every call's device counters
(itwTestBc7CallCounters: the pilot's counts and verdict, the six rotation lists, the blocks listed for modes 1/3, the pairs, the overflow words and
the deferred blocks, per band) as JSON.  Run from a build of the PARENT commit it gives tests/golden/bc7_bound_kernel_parent_counters.json: which
blocks are listed, paired and deferred is a property of the content and of the routes' rules, not of which kernel runs the 64 bounds, so a build
that moves the tail of bc7_finish_all<10> into bc7_bound_list has to reproduce every count.  (The parent's itwTestBc7CallCounters reported two-band
calls only; its counts were taken from the parent's csrc/bc7.hip with nothing changed but that hook, which now snapshots calls without bands too.)  Each case is encoded twice; a count on which the two calls
disagree is left out of the record.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bc7_waits_counters as waits  # noqa: E402

# rows x columns.  516 x 604: 76.1 chunks of 256 blocks, two bands, a ragged last workgroup whose idle lanes must reach the claim's barriers;
# 96 x 128: 3 chunks, the single-band route without a pilot; 8 x 12: 6 blocks, one workgroup with 250 idle lanes
SIZES = ((516, 604), (96, 128), (8, 12))
CONTENTS = ("smooth", "ramp_half", "channel", "baboon")
SWITCHES = ("ITW_BC7_ROT_TASKS", "ITW_BC7_PAIRS", "ITW_BC7_PAIR_CAP")
# the launch switches of one call: ITW_BC7_ROT_TASKS x ITW_BC7_PAIRS, and a bucket capacity of one pair (every bucket with two survivors overflows)
ROUTES = (("rot1-pairs1", {"ITW_BC7_ROT_TASKS": "1", "ITW_BC7_PAIRS": "1"}), ("rot1-pairs0", {"ITW_BC7_ROT_TASKS": "1", "ITW_BC7_PAIRS": "0"}),
          ("rot0-pairs1", {"ITW_BC7_ROT_TASKS": "0", "ITW_BC7_PAIRS": "1"}), ("rot0-pairs0", {"ITW_BC7_ROT_TASKS": "0", "ITW_BC7_PAIRS": "0"}),
          ("rot1-cap1", {"ITW_BC7_ROT_TASKS": "1", "ITW_BC7_PAIRS": "1", "ITW_BC7_PAIR_CAP": "1"}))


def pilots(name):
    """the pilot's thresholds a content runs under: the photograph with the pilot forced to each verdict (0: the reference's order, where
    bc7_bound_list returns at once; 100: the bounded order), the others with the bounded order forced (a surface without bands has no pilot)"""
    return (0, 100) if name == "baboon" else (100,)


def left_columns(w):
    """the width of the left half of a two-part surface: whole blocks"""
    return (w // 8) * 4


def ramp(h, w):
    """a noiseless colour ramp: the 16 texels of every block are 16 different points of one line of RGB, what mode 6's 4-bit indices are for"""
    y, x = np.mgrid[0:h, 0:w]
    v = 3 * (x % 4) + 12 * (y % 4) + 5 * ((x // 4 + y // 4) % 40)
    img = np.empty((h, w, 4), np.uint8)
    img[..., 0] = v
    img[..., 1] = v + 9
    img[..., 2] = 255 - v
    img[..., 3] = 255
    return img


def surface(name, golden_inputs, h, w):
    from itw_amd import surfaces
    if name in ("smooth", "baboon"):
        return waits.surface(name, golden_inputs, h, w)
    if name == "ramp_half":
        # left: the ramp (mode 6 runs and wins); right: the bench surface's generator, which also keeps every 32nd block column of the left half,
        # so that no 64 consecutive blocks -- no wave -- are all the ramp's even where the left half is wider than 64 blocks
        gen = surfaces.ldr_smooth(h, w)
        img = gen.copy()
        c = left_columns(w)
        img[:, :c] = ramp(h, c)
        for bx in range(31, c // 4, 32):
            img[:, 4 * bx:4 * bx + 4] = gen[:, 4 * bx:4 * bx + 4]
        return np.ascontiguousarray(img)
    if name == "channel":                                      # red and green follow x, blue follows y alone: a scalar channel for modes 4/5
        y, x = np.mgrid[0:h, 0:w]
        img = np.empty((h, w, 4), np.uint8)
        img[..., 0] = 8 * (x % 32)
        img[..., 1] = 8 * (x % 32)
        img[..., 2] = (37 * (y % 7) + 11 * ((y // 4) % 5)) % 256
        img[..., 3] = 255
        return img
    raise ValueError(name)


def key(name, h, w, pilot, route):
    return f"{name}/{h}x{w}/pilot={pilot}/{route}"


def block_modes(blocks):
    """the BC7 mode of every 16-byte block: the position of the lowest set bit of its first byte"""
    first = np.asarray(blocks, np.uint8).reshape(-1, 16)[:, 0].astype(np.int32)
    return np.array([(int(v) & -int(v)).bit_length() - 1 for v in first], np.int32)


def encode(itw, T, gpu, src, env, pilot, settings=None):
    """one `slow` call through the hooks build T (deep path set, counters armed) -> (blocks, the call's device counters by name)"""
    import torch
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    T.itwSetBc7Pilot(-2 if pilot is None else pilot)
    try:
        h, w = src.shape[:2]
        out = torch.empty((h // 4) * (w // 4) * 16, dtype=torch.uint8, device=gpu)
        st = settings if settings is not None else itw.bc7_profile("slow")
        with torch.cuda.device(gpu):
            T.itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
            surf = itw.RgbaSurface(src.data_ptr(), w, h, src.stride(0))
            T.CompressBlocksBC7(C.byref(surf), out.data_ptr(), C.byref(st))
        torch.cuda.synchronize()
        err = T.itwLastError()
        assert not err, err
        buf = (C.c_int32 * len(itw.abi.BC7_CALL_COUNTERS))()
        T.itwTestBc7CallCounters(buf, len(buf))
        return out.cpu().numpy(), dict(zip(itw.abi.BC7_CALL_COUNTERS, (int(v) for v in buf)))
    finally:
        T.itwSetBc7Pilot(-2)
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def main(out_path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "intel-texture-works-plugin_amd")]
    import torch
    import itw_amd
    gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "inputs.npz")))
    gpu = torch.device("cuda:0")
    torch.cuda.set_device(gpu)
    T = itw_amd.test_lib()
    T.itwSetBc7Path(itw_amd.abi.BC7_PATH["deep"])
    T.itwTestBc7CallCountersArm(1)
    result = {}
    for h, w in SIZES:
        for name in CONTENTS:
            src = torch.from_numpy(surface(name, gold, h, w)).to(gpu)
            for pilot in pilots(name):
                for route, env in ROUTES:
                    _, first = encode(itw_amd, T, gpu, src, env, pilot)
                    _, again = encode(itw_amd, T, gpu, src, env, pilot)
                    # a count that two calls of one build do not agree on is no property of the content: it is left out
                    result[key(name, h, w, pilot, route)] = {k: v for k, v in first.items() if again[k] == v}
    with open(out_path, "w") as f:
        json.dump({"what": "BC7 slow, deep path, the hooks library of the commit before bc7_bound_list (its counter hook reporting calls without bands "
                           "too): itwTestBc7CallCounters per surface, pilot threshold and launch switches (tools/bc7_bound_kernel_counters.py)", "counters": result}, f, indent=1, sort_keys=True)
    print("wrote", out_path, len(result), "records")


if __name__ == "__main__":
    main(sys.argv[1])
