"""Surfaces of tests/test_gpu_bc7_f02_cache.py (numpy and the oracle's from-spec decoder only), and the condition its third content is there for.

partitions(h, w): blocks of tests/_encode_sweep.py's bc7_source() -- a block decoded from (mode, partition) with a random payload is exactly
representable there -- restricted to modes 0 and 2 and laid out so that every run of 80 consecutive blocks holds each of the 16 + 64
(mode, partition) combinations once, with the payloads taking turns.  An exhaustive profile then lets every three-subset shape win mode 2, and
each of the first 16 mode 0, somewhere on any surface of 80 blocks or more; missing_winners() reads that off a stream."""
import numpy as np

import _encode_sweep as es

PROFILES = ("slow", "alpha_slow")
COMBINATIONS = [(0, p) for p in range(16)] + [(2, p) for p in range(64)]


def _pool():
    """(PAYLOADS * 80, 4, 4, 4) uint8: payload-major, the 80 combinations in COMBINATIONS' order within a payload"""
    src = es.bc7_source()
    bx = es.WIDTH // 4
    first = {}
    i = 0
    for m, fb in enumerate(es.sweep.BC7_FIELD_BITS):               # bc7_words()' order: mode, field value, payload
        first[m] = i
        i += (1 << fb) * es.PAYLOADS
    out = []
    for k in range(es.PAYLOADS):
        for m, p in COMBINATIONS:
            b = first[m] + p * es.PAYLOADS + k
            y, x = 4 * (b // bx), 4 * (b % bx)
            out.append(src[y:y + 4, x:x + 4])
    return np.stack(out)


def partitions(h, w):
    """(h, w, 4) uint8: raster block i is block i % (PAYLOADS * 80) of the pool"""
    pool = _pool()
    by, bx = h // 4, w // 4
    blocks = pool[np.arange(by * bx) % len(pool)].reshape(by, bx, 4, 4, 4)
    return np.ascontiguousarray(blocks.transpose(0, 2, 1, 3, 4).reshape(h, w, 4))


def noise(h, w, seed=20261020):
    """uniform noise in R, G, B, opaque: every shape's error is different from every other's"""
    img = np.random.default_rng(seed).integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    img[..., 3] = 255
    return img


def missing_winners(stream):
    """the (mode, partition) combinations of modes 0 and 2 that no block of a BC7 stream was encoded with"""
    return set(COMBINATIONS) - set(es.bc7_combination(stream))
