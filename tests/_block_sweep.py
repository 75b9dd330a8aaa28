"""Deterministic block streams that contain every structural combination of every format the decoders read (pure numpy, one seed).

A decoder can be wrong for one partition of one mode and right everywhere else; random bits and encoder output reach such a combination
only by chance.  These generators enumerate them instead:

  bc7()         every mode with every value of the field behind its prefix (partition; rotation + index selector), and the reserved block
  bc6h()        every value of the five mode bits with every value of the five partition bits (bits 77..81)
  bc4(signed)   every endpoint byte pair, every one of its eight levels
  bc5(signed)   the same, the second channel with the bytes swapped
  bc1(), bc3()  endpoint colours at the ends and the middle of every 565 field, in every order; bc3 with sampled alpha blocks

Each returns (blocks, width, height): a flat uint8 array of width/4 x height/4 blocks in raster order, width and height multiples of 4.
bc7_modes() and bc6h_modes() give the mode each block was built as (-1: reserved), from the construction, not from a decode.
"""
import numpy as np

SEED = 20261018
FILLS = 8                                                        # per combination: 0, ~0, 0x55.., 0xAA.., four random words
_ALL = (1 << 128) - 1
BC7_FIELD_BITS = (4, 6, 6, 6, 3, 2, 0, 6)                        # the field at bit m + 1 of mode m
BC7_COMBINATIONS = sum(1 << b for b in BC7_FIELD_BITS)           # 285
BC7_SIZE = (256, 144)                                            # 64 x 36 = 2 304 blocks
BC6H_SIZE = (256, 512)                                           # 64 x 128 = 8 192 blocks
# The format's mode prefixes in the order the decoders number the modes 0..13; two-bit prefixes (modes 0, 1) leave bits 2..4 to the payload.
BC6H_PREFIX = (0x00, 0x01, 0x02, 0x06, 0x0A, 0x0E, 0x12, 0x16, 0x1A, 0x1E, 0x03, 0x07, 0x0B, 0x0F)
BC6H_TWO_REGION_MODES = 10                                       # modes 0..9 carry a partition in bits 77..81
BC6H_RESERVED = (0x13, 0x17, 0x1B, 0x1F)
BC45_INDEX = sum((k & 7) << (3 * k) for k in range(16))          # texel k takes index k & 7


def _fills(rng):
    return [0, _ALL, _ALL // 3, _ALL // 3 * 2] + [int.from_bytes(rng.bytes(16), "little") for _ in range(4)]


def _pack(words):
    return np.frombuffer(b"".join(w.to_bytes(16, "little") for w in words), dtype=np.uint8).copy()


def _bc7_words():
    """[(mode or -1, field value, 128-bit word)] in stream order, before padding."""
    rng = np.random.default_rng(SEED)
    out = []
    for m, fb in enumerate(BC7_FIELD_BITS):
        head = (1 << (m + 1 + fb)) - 1                           # prefix and field
        for v in range(1 << fb):
            for f in _fills(rng):
                out.append((m, v, (f & ~head) | (1 << m) | (v << (m + 1))))
    for f in _fills(rng):
        out.append((-1, 0, f & ~0xFF))                           # byte 0 == 0: no mode bit, reserved
    return out


def bc7():
    words = [w for _, _, w in _bc7_words()]
    n = (BC7_SIZE[0] // 4) * (BC7_SIZE[1] // 4)
    assert len(words) == (BC7_COMBINATIONS + 1) * FILLS <= n
    return _pack(words + [words[0]] * (n - len(words))), BC7_SIZE[0], BC7_SIZE[1]


def bc7_modes():
    modes = [m for m, _, _ in _bc7_words()]
    n = (BC7_SIZE[0] // 4) * (BC7_SIZE[1] // 4)
    return np.array(modes + [modes[0]] * (n - len(modes)), dtype=np.int32)


def _bc6h_words():
    """[(mode or -1, low five bits, bits 77..81, 128-bit word)] in stream order."""
    rng = np.random.default_rng(SEED + 1)
    keep = _ALL & ~0x1F & ~(0x1F << 77)
    out = []
    for low in range(32):
        key = low & 3 if (low & 3) < 2 else low
        mode = BC6H_PREFIX.index(key) if key in BC6H_PREFIX else -1
        for part in range(32):
            for f in _fills(rng):
                out.append((mode, low, part, (f & keep) | low | (part << 77)))
    return out


def bc6h():
    words = [w for _, _, _, w in _bc6h_words()]
    assert len(words) == (BC6H_SIZE[0] // 4) * (BC6H_SIZE[1] // 4)
    return _pack(words), BC6H_SIZE[0], BC6H_SIZE[1]


def bc6h_modes():
    return np.array([m for m, _, _, _ in _bc6h_words()], dtype=np.int32)


def _bc4_blocks(swap):
    pair = np.arange(65536)
    b = np.empty((65536, 8), dtype=np.uint8)
    b[:, 1 if swap else 0] = pair >> 8
    b[:, 0 if swap else 1] = pair & 255
    b[:, 2:] = np.frombuffer(BC45_INDEX.to_bytes(6, "little"), dtype=np.uint8)
    return b


def bc4(signed=False):
    """All 65 536 endpoint byte pairs, block i = (i >> 8, i & 255).  The bytes are the same for BC4_UNORM and BC4_SNORM: all pairs of
    bytes are all pairs of either reading; `signed` names the reading for the caller's sake."""
    return _bc4_blocks(False).reshape(-1), 1024, 1024


def bc5(signed=False):
    return np.concatenate([_bc4_blocks(False), _bc4_blocks(True)], axis=1).reshape(-1), 1024, 1024


def _rgb565_corners():
    """The 125 colours whose fields each take a value from {0, 1, middle, max - 1, max}."""
    r5, g6 = (0, 1, 15, 30, 31), (0, 1, 31, 62, 63)
    return np.array([(r << 11) | (g << 5) | b for r in r5 for g in g6 for b in r5], dtype=np.uint32)


def _colour_blocks():
    c = _rgb565_corners()
    c0, c1 = np.repeat(c, c.size), np.tile(c, c.size)            # every ordered pair: c0 > c1, c0 == c1, c0 < c1
    b = np.empty((c0.size, 8), dtype=np.uint8)
    b[:, 0], b[:, 1], b[:, 2], b[:, 3] = c0 & 255, c0 >> 8, c1 & 255, c1 >> 8
    b[:, 4:] = 0xE4                                              # indices 0, 1, 2, 3 along each row
    return b


def bc1():
    return _colour_blocks().reshape(-1), 500, 500


def bc3():
    colour = _colour_blocks()
    rng = np.random.default_rng(SEED + 3)
    alpha = np.empty((colour.shape[0], 8), dtype=np.uint8)
    alpha[:, :2] = rng.integers(0, 256, size=(colour.shape[0], 2))
    alpha[:256, 0] = alpha[:256, 1] = np.arange(256)             # a0 == a1 at every value; the rest falls on both sides
    alpha[:, 2:] = np.frombuffer(BC45_INDEX.to_bytes(6, "little"), dtype=np.uint8)
    return np.concatenate([alpha, colour], axis=1).reshape(-1), 500, 500
