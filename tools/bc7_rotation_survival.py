"""How many (block, rotation) pairs of modes 4/5 an exact bound leaves under an RGB profile (csrc/bc7.hip, bc7_rot_tasks) -- on the CPU.
A mode 4/5 candidate of rotation p (channels == 3) codes the two channels it keeps as rounded points of ONE segment and channel p on its
own (error >= 0), so its error is >= (sqrt(R2(p)) - sqrt(2)/2 sqrt(16))_+^2 with R2(p) the residual of the 16 texels about their best
line in the two kept channels = trace - largest eigenvalue of that 2x2 part of the whole-block scatter matrix.
  rotation_bounds_f32   the bound in the form the device uses (csrc/bc7_exact.hpp rotation_bound): float32, 16 x R2 = det / largest eigenvalue with the
                        determinant an exact 64-bit integer, a relative margin of 1e-5, 0.999999 factors, the slack rounded up
  rotation_bounds_f64   the same number in float64 without margins (what the float32 form must never exceed)
  survivors             !(bound >= e02 - 0.5): e02 = the error modes 0/2 leave (the oracle with mode_selection = (1,0,0,0)); errors are
                        integers and modes 4/5 replace a block only on a strict `<`
usage: python tools/bc7_rotation_survival.py [side of the bench surface's crop, default 1024] > profiles/r09_bc7_rotation_survival.txt"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "intel-texture-works-plugin_amd"))

SLACK2_16 = np.float32(2.82842732)       # sqrt(2)/2 sqrt(16), rounded up (csrc/bc7_exact.hpp BOUND_SLACK2_16)
KEPT = ((1, 2), (0, 2), (0, 1))          # rotation p keeps the other two channels


def blocks_of(img):
    """(H, W, 4) uint8 -> (blocks, 16, 3) int64, raster block order"""
    h, w = img.shape[0] // 4 * 4, img.shape[1] // 4 * 4
    return img[:h, :w, :3].astype(np.int64).reshape(h // 4, 4, w // 4, 4, 3).transpose(0, 2, 1, 3, 4).reshape(-1, 16, 3)


def scatter16(blk):
    """16 x the scatter matrix of each block's 16 texels, exact integers below 2^24: (blocks, 3, 3)"""
    s = blk.sum(axis=1)
    m = np.einsum("bki,bkj->bij", blk, blk)
    return 16 * m - s[:, :, None] * s[:, None, :]


def rotation_bounds_f32(blk):
    """(blocks, 3) float32: the device's arithmetic, operation by operation (numpy rounds every float32 operation once)"""
    f = np.float32
    c = scatter16(blk)
    out = np.zeros((blk.shape[0], 3), f)
    for p, (i, j) in enumerate(KEPT):
        det = (c[:, i, i] * c[:, j, j] - c[:, i, j] * c[:, i, j]).astype(f)     # exact in 64-bit integers, rounded once
        t = (c[:, i, i] + c[:, j, j]).astype(f)
        dif, b = (c[:, i, i] - c[:, j, j]).astype(f), c[:, i, j].astype(f)
        lam = f(0.5) * (t + np.sqrt(dif * dif + f(4.0) * (b * b)))
        res = (det * (f(1.0) / np.maximum(lam, f(1.0)))) * f(0.99999)            # 16 x R2(p), from below
        dist = np.sqrt(res * f(0.0625)) * f(0.999999) - SLACK2_16
        e = np.maximum(dist, f(0.0))
        out[:, p] = e * e * f(0.999999)
    return out


def rotation_bounds_f64(blk):
    c = scatter16(blk).astype(np.float64)
    out = np.zeros((blk.shape[0], 3))
    for p, (i, j) in enumerate(KEPT):
        sub = c[:, [i, j]][:, :, [i, j]]
        lam = np.linalg.eigvalsh(sub)[:, 1]
        r2 = np.maximum(sub[:, 0, 0] + sub[:, 1, 1] - lam, 0.0) / 16.0
        out[:, p] = np.maximum(np.sqrt(r2) - np.sqrt(2.0) / 2.0 * 4.0, 0.0) ** 2
    return out


def errors_02(img):
    """per block the error the oracle's modes {0,2} leave under `slow` (raster block order)"""
    from oracle import pyoracle
    L = pyoracle.lib()
    L.oracle_bc7_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.oracle_bc7_block.restype = None
    s = pyoracle.bc7_profile("slow")
    s.mode_selection[0], s.mode_selection[1], s.mode_selection[2], s.mode_selection[3] = 1, 0, 0, 0
    h, w = img.shape[0] // 4 * 4, img.shape[1] // 4 * 4
    planar = np.ascontiguousarray(img[:h, :w].astype(np.float32).reshape(h // 4, 4, w // 4, 4, 4).transpose(0, 2, 4, 1, 3).reshape(-1, 64))
    data = (C.c_uint32 * 4)()
    e = C.c_float()
    out = np.zeros(planar.shape[0], np.int64)
    for k, blk in enumerate(planar):
        L.oracle_bc7_block(blk.ctypes.data, C.byref(s), data, C.byref(e))
        out[k] = int(e.value)
    return out


def survivors(bounds, e02):
    return ~(bounds >= (e02.astype(np.float32) - np.float32(0.5))[:, None])


def row(name, img):
    blk = blocks_of(img)
    sv = survivors(rotation_bounds_f32(blk), errors_02(img))
    k = sv.sum(axis=1)
    print(f"{name:24s} {blk.shape[0]:7d}   {sv[:, 0].mean():.3f} / {sv[:, 1].mean():.3f} / {sv[:, 2].mean():.3f}   {sv.mean():9.3f}   "
          f"{(k == 0).mean():.3f} / {(k == 1).mean():.3f} / {(k == 2).mean():.3f} / {(k == 3).mean():.3f}")
    return sv.mean()


def main():
    from itw_amd import surfaces
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    z = np.load(os.path.join(ROOT, "tests", "golden", "inputs.npz"))
    bench = np.ascontiguousarray(surfaces.ldr_smooth(4096, 4096, surfaces.SEED)[1024:1024 + side, 2048:2048 + side])
    baboon, monkey = z["baboon"], z["monkey"]
    hb = min(bench.shape[0], baboon.shape[0]) // 4 * 4
    wb = min(bench.shape[1], baboon.shape[1]) // 4 * 4
    mix = np.ascontiguousarray(np.concatenate([bench[:hb, :wb], baboon[:hb, :wb]], axis=0))
    print("# tools/bc7_rotation_survival.py: `slow`, the float32 bound of the device (csrc/bc7_exact.hpp rotation_bound) against the error modes {0,2} leave")
    print("# a (block, rotation) pair survives when !(bound >= e02 - 0.5): only those pairs can change a block through modes 4/5")
    print(f"{'content':24s} {'blocks':>7s}   {'rotation 0 / 1 / 2':21s}   {'all pairs':>9s}   blocks with 0 / 1 / 2 / 3 surviving rotations")
    s = row(f"bench surface {side}^2 crop", bench)
    row("baboon", baboon)
    row("monkey", monkey)
    row("half bench / half baboon", mix)
    print(f"# go / no-go: {s:.3f} of the bench surface's pairs survive; the route pays at or below 0.65 -> {'GO' if s <= 0.65 else 'NO-GO'}")


if __name__ == "__main__":
    main()
