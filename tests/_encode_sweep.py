"""Source images on which every structural combination of BC7 and BC6H wins an encode (numpy and the oracle's from-spec decoders only).

An encoder can be wrong for one partition of one mode and right everywhere else, and which (mode, partition) pairs it searches, wins with and
writes out is otherwise left to the content.  A block decoded from a combination with a random payload is exactly representable in that
combination, so an exhaustive profile reproduces it with error 0 there (or in a mode earlier in the reference's order that reaches 0 too):

  bc7_source()      every mode with every value of the field behind its prefix (tests/_block_sweep.py's construction), PAYLOADS random payloads
                    each, decoded: RGBA8, 256 wide
  bc6h_source()     every valid mode, modes 0..9 with every partition, PAYLOADS random payloads each, followed by the valid blocks of
                    _block_sweep.bc6h() (all-zero, all-one, alternating and random payloads), decoded: RGBA16F with alpha 0x3C00, 256 wide
  small_sources()   _block_sweep's BC1 / BC3 / BC4 / BC5 streams decoded: every texel on an interpolation level of all 65 536 BC4 / BC5 endpoint
                    pairs and of the 565 corner colours in both orders

bc7_combination() and bc6h_combination() read the (mode, field) pair of each block of a stream from the format's bit layout.
"""
import numpy as np

import _block_sweep as sweep

SEED = 20261020
PAYLOADS = 16                                                    # per combination
WIDTH = 256
BC7_COMBINATIONS = sweep.BC7_COMBINATIONS                        # 285
BC6H_COMBINATIONS = sweep.BC6H_TWO_REGION_MODES * 32 + 4         # 324: ten two-region modes x 32 partitions, four one-region modes
_ALL = (1 << 128) - 1
_cache = {}


def _oracle():
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle


def _random_word(rng):
    return int.from_bytes(rng.bytes(16), "little")


def _padded(words):
    """Whole rows of WIDTH / 4 blocks, the last one filled by repeating the first block."""
    per_row = WIDTH // 4
    n = -(-len(words) // per_row) * per_row
    return sweep._pack(words + [words[0]] * (n - len(words))), n // per_row * 4


def bc7_words():
    """[(mode, field value, 128-bit word)]: prefix and field as given, every bit above them drawn."""
    rng = np.random.default_rng(SEED)
    out = []
    for m, fb in enumerate(sweep.BC7_FIELD_BITS):
        head = (1 << (m + 1 + fb)) - 1
        for v in range(1 << fb):
            for _ in range(PAYLOADS):
                out.append((m, v, (_random_word(rng) & ~head) | (1 << m) | (v << (m + 1))))
    return out


def bc6h_words():
    """[(mode, partition or 0, 128-bit word)]: the drawn blocks, then the valid ones of _block_sweep.bc6h()."""
    rng = np.random.default_rng(SEED + 1)
    out = []
    for mode, prefix in enumerate(sweep.BC6H_PREFIX):
        head = 3 if mode < 2 else 31                             # modes 0 and 1 have two prefix bits; bits 2..4 are payload
        if mode < sweep.BC6H_TWO_REGION_MODES:
            keep = _ALL & ~head & ~(0x1F << 77)
            for part in range(32):
                for _ in range(PAYLOADS):
                    out.append((mode, part, (_random_word(rng) & keep) | prefix | (part << 77)))
        else:                                                    # one region: bits 77..81 are index bits
            for _ in range(PAYLOADS):
                out.append((mode, 0, (_random_word(rng) & ~head) | prefix))
    for mode, _, part, word in sweep._bc6h_words():
        if mode >= 0:
            out.append((mode, part if mode < sweep.BC6H_TWO_REGION_MODES else 0, word))
    return out


def _frozen(img):
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


def bc7_source():
    """(H, 256, 4) uint8, read-only; block i of the first 285 * PAYLOADS decodes bc7_words()[i]."""
    if "bc7" not in _cache:
        blocks, h = _padded([w for _, _, w in bc7_words()])
        img, modes = _oracle().decode("bc7", blocks, WIDTH, h)
        assert (modes >= 0).all()
        _cache["bc7"] = _frozen(img)
    return _cache["bc7"]


def bc6h_source():
    """(H, 256, 4) uint16 half bits, read-only, alpha 0x3C00."""
    if "bc6h" not in _cache:
        blocks, h = _padded([w for _, _, w in bc6h_words()])
        rgb, modes = _oracle().decode("bc6h", blocks, WIDTH, h)
        assert (modes >= 0).all() and int(rgb.max()) <= 0x7BFF   # finite halves only
        img = np.empty((h, WIDTH, 4), dtype=np.uint16)
        img[..., :3] = rgb
        img[..., 3] = 0x3C00
        _cache["bc6h"] = _frozen(img)
    return _cache["bc6h"]


def small_sources():
    """{"bc1" | "bc3" | "bc4" | "bc5": (H, W, 4) uint8, read-only}: 500 x 500 for BC1 / BC3, 1024 x 1024 for BC4 / BC5."""
    if "small" not in _cache:
        out = {}
        for fmt in ("bc1", "bc3", "bc4", "bc5"):
            blocks, w, h = getattr(sweep, fmt)()
            out[fmt] = _frozen(_oracle().decode(fmt, blocks, w, h)[0])
        _cache["small"] = out
    return _cache["small"]


# ---- settings structs on top of a preset: {name: (preset, {field: value})}; "mode_selection" takes all four flags -----------------------

BC7_VARIANTS = {}
for _n in (16, 17, 1, 64):                                       # 16: the in-register ranking; 17: LDS keys and the per-family kernels
    BC7_VARIANTS[f"thresholds_{_n}"] = ("alpha_slow", {"fastSkipTreshold_mode1": _n, "fastSkipTreshold_mode3": _n, "fastSkipTreshold_mode7": _n})
for _k, _family in enumerate(("modes_02", "modes_137", "modes_45", "mode_6")):
    BC7_VARIANTS[f"only_{_family}"] = ("alpha_slow", {"mode_selection": tuple(int(i == _k) for i in range(4))})
for _c in range(4):
    BC7_VARIANTS[f"channel0_{_c}"] = ("alpha_slow", {"mode45_channel0": _c})
BC6H_VARIANTS = {f"list_{n}_refine2p_{r}": ("slow", {"fastSkipTreshold": n, "refineIterations_2p": r}) for n in (1, 2, 31, 32) for r in (0, 2)}


def apply(settings, tweak):
    """The tweak of a variant written into a settings struct (the product's or the oracle's: same fields)."""
    for k, v in tweak.items():
        if k == "mode_selection":
            for i in range(4):
                settings.mode_selection[i] = v[i]
        else:
            setattr(settings, k, v)
    return settings


# ---- reading a stream: the formats' bit layouts, no decoder ----------------------------------------------------------------------------

_BC7_FIELD_BITS = {0: 4, 1: 6, 2: 6, 3: 6, 4: 3, 5: 2, 6: 0, 7: 6}
_BC6H_MODE = {0x00: 0, 0x01: 1, 0x02: 2, 0x06: 3, 0x0A: 4, 0x0E: 5, 0x12: 6, 0x16: 7, 0x1A: 8, 0x1E: 9, 0x03: 10, 0x07: 11, 0x0B: 12, 0x0F: 13}


def _words(blocks):
    return [int.from_bytes(b.tobytes(), "little") for b in np.asarray(blocks, dtype=np.uint8).reshape(-1, 16)]


def bc7_combination(blocks):
    """Per block (mode, field): the mode is the number of zero bits below the lowest set bit of byte 0, the field the partition (modes 0..3, 7),
    rotation + index selector (mode 4) or rotation (mode 5) in the bits that follow; (-1, 0) for a reserved block."""
    out = []
    for v in _words(blocks):
        if v & 0xFF == 0:
            out.append((-1, 0))
            continue
        m = (v & -v).bit_length() - 1
        out.append((m, (v >> (m + 1)) & ((1 << _BC7_FIELD_BITS[m]) - 1)))
    return out


def bc6h_combination(blocks):
    """Per block (mode 0..13, partition): two prefix bits if they read 0 or 1, five otherwise; the partition is bits 77..81 of the two-region
    modes 0..9 and 0 for the one-region modes 10..13; (-1, 0) for a reserved prefix."""
    out = []
    for v in _words(blocks):
        low = v & 31
        mode = _BC6H_MODE.get(low & 3 if (low & 3) < 2 else low, -1)
        out.append((mode, (v >> 77) & 31 if 0 <= mode < 10 else 0))
    return out


def all_bc7_combinations():
    return {(m, v) for m, fb in _BC7_FIELD_BITS.items() for v in range(1 << fb)}


def all_bc6h_combinations():
    return {(m, p) for m in range(10) for p in range(32)} | {(m, 0) for m in range(10, 14)}
