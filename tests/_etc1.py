"""Shared by the ETC1 tests (tests/test_etc1_cpu.py, tests/test_gpu_etc1.py) and tools/gen_golden_etc1.py: the two seeded inputs, a ctypes
call of the reference library's CompressBlocksETC1 (oracle/_ref/libispc_texcomp_ref_full.so: the reference's own kernel source built as
one scalar program instance), and an ETC1 decoder written in numpy from the format's definition (OES_compressed_ETC1_RGB8_texture) --
independent of both the encoder under test and the device decoder."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_etc1.npz")
GOLDEN_THRESHOLDS = (1, 6, 32, 165)
ETC1 = 0x8D64

# {small, large} of the eight modifier tables; a texel's modifier is (small, large, -small, -large)[msb * 2 + lsb]
MODIFIERS = np.array([[2, 8], [5, 17], [9, 29], [13, 42], [18, 60], [24, 80], [33, 106], [47, 183]], dtype=np.int32)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def noise(seed=2):
    """64 x 64 RGBA8, uniform random bytes."""
    return np.random.default_rng(seed).integers(0, 256, (64, 64, 4), dtype=np.uint8)


def ramp(seed=3):
    """64 x 64 RGBA8: a random colour per block plus noise whose amplitude grows from +-1 at the left edge to +-128 at the right, clipped; alpha 255."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (16, 16, 3)).repeat(4, axis=0).repeat(4, axis=1)
    amp = np.rint(1 + 127 * np.arange(64) / 63.0).astype(np.int64)[None, :, None]
    jitter = rng.integers(-128, 129, (64, 64, 3)) * amp // 128
    img = np.full((64, 64, 4), 255, dtype=np.uint8)
    img[..., :3] = np.clip(base + jitter, 0, 255)
    return img


# ---- the reference library ------------------------------------------------------------------------------------------------------------------
class _Surface(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32)]


class _Settings(C.Structure):
    _fields_ = [("fastSkipTreshold", C.c_int)]


_ref = None
_streams = {}


def ref_path():
    return os.path.join(ROOT, "oracle", "_ref", "libispc_texcomp_ref_full.so")


def ref_lib():
    global _ref
    if _ref is None:
        _ref = C.CDLL(ref_path(), mode=os.RTLD_LOCAL)
        _ref.CompressBlocksETC1.argtypes = [C.POINTER(_Surface), C.c_void_p, C.POINTER(_Settings)]
        _ref.CompressBlocksETC1.restype = None
        _ref.GetProfile_etc_slow.argtypes = [C.c_void_p]
        _ref.GetProfile_etc_slow.restype = None
    return _ref


def live_reference():
    """The reference library.  It is a build product (build() makes it next to the reference tree, and it travels with the tree to the GPU
    box), so its absence is a failure, not a skip: a silent skip would turn every comparison with it green.  ITW_ALLOW_NO_REF=1 downgrades
    the failure to a skip for a deliberate run without it, as for tests/test_gpu_vs_reference_kernel.py; the golden-file tests need no binary."""
    import pytest
    if not os.path.exists(ref_path()):
        if os.environ.get("ITW_ALLOW_NO_REF") == "1":
            pytest.skip("oracle/_ref/libispc_texcomp_ref_full.so absent and ITW_ALLOW_NO_REF=1")
        pytest.fail("oracle/_ref/libispc_texcomp_ref_full.so is missing (build() / make -C oracle/ref_build makes it; "
                    "or set ITW_ALLOW_NO_REF=1 to run without the comparisons with the live reference)")
    return ref_lib()


def ref_encode(img, threshold):
    """The reference's block stream of img ((H, W, 4) uint8, rows may be strided) at fastSkipTreshold = threshold (1 .. 165)."""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 4 and img.strides[1] == 4 and img.strides[2] == 1 and 1 <= threshold <= 165
    h, w = img.shape[:2]
    out = np.zeros((h // 4) * (w // 4) * 8, dtype=np.uint8)
    surf = _Surface(img.ctypes.data, w, h, img.strides[0])
    st = _Settings(threshold)
    ref_lib().CompressBlocksETC1(C.byref(surf), out.ctypes.data, C.byref(st))
    return out


def ref_stream(name, threshold):
    """ref_encode of the input `name` ('noise' / 'ramp'), computed once per process."""
    key = (name, threshold)
    if key not in _streams:
        _streams[key] = ref_encode({"noise": noise, "ramp": ramp}[name](), threshold)
        _streams[key].setflags(write=False)
    return _streams[key]


# ---- the golden file ------------------------------------------------------------------------------------------------------------------------
def sha256(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load_golden():
    """tests/golden/golden_etc1.npz as a dict: 'ramp' and 'noise' (the inputs), '<input>.t<threshold>' (the reference's streams) and
    '<input>.t<threshold>.psnr'.  The file holds the ramp, the streams and the PSNRs; the noise input is 16 KiB that no compressor
    shortens, so the file keeps its SHA-256 instead and noise() regenerates it here -- a generator that ever produced other bytes fails
    this check instead of comparing the wrong surface with the stored streams."""
    g = dict(np.load(GOLDEN))
    img = noise()
    assert sha256(img) == str(g["noise.sha256"]), "noise() no longer generates the surface the golden streams were made from"
    g["noise"] = img
    return g


# ---- the format, from its definition ----------------------------------------------------------------------------------------------------------
def fields(blocks):
    """The header fields of every block: dict of int32 arrays -- flip, diff, table0, table1, base (n, 3): the 4- or 5-bit first base,
    second (n, 3): the second 4-bit base, or the 3-bit delta as a signed number."""
    b = np.asarray(blocks, dtype=np.uint8).reshape(-1, 8).astype(np.int32)
    diff = (b[:, 3] >> 1) & 1
    rgb = b[:, :3]
    delta = rgb & 7
    delta = delta - ((delta & 4) << 1)
    return {"flip": b[:, 3] & 1, "diff": diff, "table0": b[:, 3] >> 5, "table1": (b[:, 3] >> 2) & 7,
            "base": np.where(diff[:, None] == 1, rgb >> 3, rgb >> 4), "second": np.where(diff[:, None] == 1, delta, rgb & 15)}


def decode_np(blocks, width, height):
    """(texels (height, width, 4) uint8 with alpha 255, modes int32) of a raster-order stream of (width / 4) * (height / 4) blocks.
    modes: 0 individual, 1 differential, -1 a differential block whose base + delta leaves 0 .. 31 (decoded with the sum modulo 32)."""
    assert width % 4 == 0 and height % 4 == 0
    f = fields(blocks)
    n = f["flip"].size
    assert n == (width // 4) * (height // 4)
    diff = f["diff"][:, None] == 1
    total = f["base"] + f["second"]
    modes = np.where(f["diff"] == 1, np.where(((total < 0) | (total > 31)).any(axis=1), -1, 1), 0).astype(np.int32)
    five0, five1 = f["base"], total & 31
    base0 = np.where(diff, (five0 << 3) | (five0 >> 2), f["base"] * 17)
    base1 = np.where(diff, (five1 << 3) | (five1 >> 2), f["second"] * 17)
    b = np.asarray(blocks, dtype=np.uint8).reshape(-1, 8).astype(np.uint32)
    msb = (b[:, 4] << 8) | b[:, 5]
    lsb = (b[:, 6] << 8) | b[:, 7]
    out = np.empty((n, 4, 4, 4), dtype=np.uint8)                 # [block, y, x, channel]
    out[..., 3] = 255
    for y in range(4):
        for x in range(4):
            bit = x * 4 + y
            second = np.where(f["flip"] == 1, y >= 2, x >= 2)
            table = np.where(second, f["table1"], f["table0"])
            m, l = (msb >> bit) & 1, (lsb >> bit) & 1
            mod = MODIFIERS[table, l] * np.where(m == 1, -1, 1)
            colour = np.where(second[:, None], base1, base0) + mod[:, None]
            out[:, y, x, :3] = np.clip(colour, 0, 255)
    bx = width // 4
    texels = out.reshape(height // 4, bx, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(height, width, 4)
    return np.ascontiguousarray(texels), modes


def psnr_rgb(a, b):
    d = a[..., :3].astype(np.int64) - b[..., :3].astype(np.int64)
    sse = int((d * d).sum())
    return float("inf") if sse == 0 else 10.0 * np.log10(255.0 ** 2 * d.size / sse)


def coverage(streams):
    """What the streams exercise: the set of (flip, diff) pairs, the tables used per half, the number of differential blocks and how many
    of them have a delta at -4 or +3 (the clamp of the second half around the first)."""
    f = fields(np.concatenate([np.asarray(s, dtype=np.uint8).reshape(-1) for s in streams]))
    d = f["diff"] == 1
    edge = ((f["second"][d] == -4) | (f["second"][d] == 3)).any(axis=1)
    return {"pairs": set(zip(f["flip"].tolist(), f["diff"].tolist())), "table0": set(f["table0"].tolist()), "table1": set(f["table1"].tolist()),
            "differential": int(d.sum()), "clamped": int(edge.sum())}
