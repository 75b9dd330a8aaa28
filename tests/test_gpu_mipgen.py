"""itwGenerateMipChain and itwCompressImageMipped on the device (include/itw_dispatch.h, "Mip chains"; csrc/mipgen.hip).  Every comparison
is == on bytes against the numpy model of tests/_mipgen.py, which tests/test_mipgen_cpu.py pins to the reference's own filters; where a
recorded case exists (tests/golden/mipgen_ref.npz, mipgen_ref_sha256.json) the device is compared with the recording directly."""
import hashlib
import json
import os

import numpy as np
import pytest

import _guarded as G
import _mipgen as M
import _normal_prep as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLD, "mipgen_ref_sha256.json")) as _f:
    PINS = json.load(_f)["cases"]


def _dev(gpu, a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(gpu)


def _np(t, dtype):
    return (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)).view(dtype)


def _half(h, w, seed):
    """Finite RGBA16F content: magnitudes 2^-12 .. 2^12 next to each other (sums that round in fp32), +-0, half denormals, +-65504 and
    quads of four 65504s (their mean must store 65504).  And exact -0 sums, the case the store's empty asm exists for (mipgen.hpp: the
    compiler's fused multiply-convert adds +0 and loses the sign): a block of -0 in all four channels, aligned to its own size, so that
    whole quads of -0 meet again one, two and three levels down -- the pyramid kernel's register levels and its first LDS level, the
    tail kernel's global and LDS levels, and the per-level kernel -- and next to it a quad [-0, -0, +0, -0], which must store +0.  A
    chain of height or width 1 or 2 gets a run of -0 instead.  _exact_zero_sums() asserts that these cases are in the expected chain."""
    rng = np.random.default_rng(seed)
    bits = M.seeded_half_image(h, w, seed)
    special = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x7BFF, 0xFBFF, 0x0400, 0x3C00], dtype=np.uint16)
    pick = rng.integers(0, 6, (h, w, 4)) == 0
    bits[pick] = special[rng.integers(0, special.size, int(pick.sum()))]
    if h >= 2 and w >= 2:
        bits[0:2, 0:2] = 0x7BFF
        bits[h - 2:h, w - 2:w] = 0xFBFF
    if min(h, w) >= 32:
        bits[8:16, 8:16] = 0x8000
        bits[16:18, 16:18] = 0x8000
        bits[17, 16] = 0x0000
    elif min(h, w) == 1 and max(h, w) == 8:
        flat = bits.reshape(-1, 4)                                # 8 x 1 or 1 x 8: the texels in order (a view)
        flat[0:4] = 0x8000
        flat[4:6] = [[0x8000] * 4, [0x0000] * 4]
    elif min(h, w) <= 2 and max(h, w) >= 64:
        wide = bits if w > h else bits.transpose(1, 0, 2)         # a view: rows of the short axis
        wide[:, 16:32] = 0x8000
        wide[:, 32:34] = 0x8000
        wide[0, 33] = 0x0000
    return bits


def _bytes(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def _content(kind, h, w, seed):
    return _half(h, w, seed) if kind == "f16" else _bytes(h, w, seed)


def _equal_chain(got, want, what):
    assert len(got) == len(want), what
    for l, (g, w) in enumerate(zip(got, want)):
        g = _np(g, w.dtype)
        assert g.shape == w.shape, (what, l, g.shape, w.shape)
        bad = np.flatnonzero((g != w).any(axis=2))
        assert bad.size == 0, (what, f"level {l}: {bad.size} texels differ, first at {divmod(int(bad[0]), w.shape[1])}: "
                               f"got {g.reshape(-1, 4)[bad[0]].tolist()} want {w.reshape(-1, 4)[bad[0]].tolist()}")


def _taps(src):
    """The four taps of every texel of the next box level (tests/_mipgen.py box_level)."""
    h, w = src.shape[:2]
    r0, r1 = (src[0::2], src[1::2]) if h > 1 else (src, src)
    c0, c1 = (slice(0, None, 2), slice(1, None, 2)) if w > 1 else (slice(None), slice(None))
    return r0[:, c0], r1[:, c0], r0[:, c1], r1[:, c1]


def _exact_zero_sums(chain):
    """Per level >= 1 of an expected RGBA16F chain: how many values are the sum of four -0 taps (they must be -0), and how many of four
    zeros that are not all negative (they must be +0).  Only an exact -0 sum keeps the sign; a tiny negative sum that underflows does not
    count."""
    neg, mixed = [], []
    for l in range(1, len(chain)):
        taps = _taps(chain[l - 1])
        all_neg = np.logical_and.reduce([t == 0x8000 for t in taps])
        all_zero = np.logical_and.reduce([(t & 0x7FFF) == 0 for t in taps]) & ~all_neg
        assert (chain[l][all_neg] == 0x8000).all() and (chain[l][all_zero] == 0x0000).all(), l
        neg.append(int(all_neg.sum()))
        mixed.append(int(all_zero.sum()))
    return neg, mixed


# levels of a box chain of _half() content that must hold an exact -0 sum: three under the 8 x 8 block, two under a run of 4, four under a run of 16 x 2
NEG_ZERO_LEVELS = {(64, 64): 3, (128, 128): 3, (256, 64): 3, (64, 256): 3, (64, 32): 3, (32, 64): 3, (32, 32): 3, (8, 1): 2, (1, 8): 2, (512, 2): 4}

BOX_SIZES = [(1, 1), (2, 2), (64, 64), (128, 128), (256, 64), (64, 256), (8, 1), (1, 8), (512, 2), (64, 32), (32, 64), (32, 32)]       # (width, height)


@pytest.mark.parametrize("kind", ["u8", "f16"])
@pytest.mark.parametrize("w,h", BOX_SIZES)
def test_box_chains_on_both_routes(itw, gpu, kind, w, h):
    """1 x 1 and 2 x 2; 64^2: one tile, all six levels; 128^2: 2 x 2 tiles then the tail kernel from 2 x 2; 256 x 64 and 64 x 256: tile counts
    differ per axis (the wide one runs on after its height has reached 1: the stated divergence); 8 x 1, 1 x 8; 512 x 2: per-level launches
    bridge to the tail kernel at 64 x 1; 64 x 32, 32 x 64, 32 x 32: the largest levels the tail kernel starts from."""
    import torch
    base = _content(kind, h, w, 100 * w + h)
    full = M.levels_of(w, h)
    want_full = M.chain(base)
    if kind == "f16" and (w, h) in NEG_ZERO_LEVELS:
        neg, mixed = _exact_zero_sums(want_full)
        assert all(n >= 4 for n in neg[:NEG_ZERO_LEVELS[(w, h)]]) and mixed[0] >= 4, ("the expected chain lost its exact -0 sums", w, h, neg, mixed)
    for levels in sorted({min(2, full), min(3, full), full}):
        want = want_full[:levels]
        routes = {}
        for per_level in (False, True):
            got = itw.generate_mips(_dev(gpu, base), levels=levels, per_level=per_level)
            torch.cuda.synchronize()
            _equal_chain(got, want, (w, h, kind, levels, "per level" if per_level else "pyramid"))
            routes[per_level] = [_np(g, base.dtype) for g in got]
        assert all(np.array_equal(a, b) for a, b in zip(routes[False], routes[True]))


@pytest.mark.parametrize("kind", ["u8", "f16"])
def test_six_items_in_one_call(itw, gpu, kind):
    import torch
    bases = [_content(kind, 128, 128, 7 + i) for i in range(6)]
    for per_level in (False, True):
        got = itw.generate_mips([_dev(gpu, b) for b in bases], per_level=per_level)
        torch.cuda.synchronize()
        for i, b in enumerate(bases):
            _equal_chain(got[i], M.chain(b), (kind, "item", i, per_level))
    host = itw.generate_mips(bases, levels=4)
    for i, b in enumerate(bases):
        _equal_chain(host[i], M.chain(b, 4), (kind, "host item", i))


def test_rgba8_box_is_the_integer_rule_at_every_remainder(itw, gpu):
    """2 x 2 quads whose a + b + c + d runs through every value mod 4 at 0, at a quarter, in mid-range (508 .. 511) and at 1020."""
    quads = []
    for lo in (0, 126, 252, 508):
        for s in range(lo, lo + 4):
            quads.append([s // 4 + (1 if k < s % 4 else 0) for k in range(4)])
    quads += [[255, 255, 255, 255], [255, 255, 255, 254], [255, 254, 255, 254], [254, 254, 255, 254], [0, 0, 0, 0], [0, 255, 0, 255], [255, 0, 0, 0]]
    sums = {sum(q) % 4 for q in quads}
    assert sums == {0, 1, 2, 3} and max(sum(q) for q in quads) == 1020 and min(sum(q) for q in quads) == 0
    assert {sum(q) for q in quads} >= {0, 1, 2, 3, 508, 509, 510, 511, 1017, 1018, 1019, 1020}
    img = np.zeros((128, 128, 4), np.uint8)
    for i in range(64 * 64):                                  # quad i of the image, channel c: quads[i + c]
        y, x = 2 * (i // 64), 2 * (i % 64)
        for c in range(4):
            img[y, x, c], img[y + 1, x, c], img[y, x + 1, c], img[y + 1, x + 1, c] = quads[(i + c) % len(quads)]
    for per_level in (False, True):
        got = itw.generate_mips(_dev(gpu, img), per_level=per_level)
        want = [img]
        for _ in range(7):
            want.append(M.box_level_rgba8_integer(want[-1]))
        _equal_chain(got, want, ("integer rule", per_level))
    _equal_chain(M.chain(img), want, "the model is the integer rule")


@pytest.mark.parametrize("name", sorted(PINS))
def test_the_device_equals_the_recorded_reference(itw, gpu, name):
    e = PINS[name]
    gold = np.load(os.path.join(GOLD, "mipgen_ref.npz"))
    base = M.seeded_half_image(e["height"], e["width"], e["seed"])
    assert hashlib.sha256(base.tobytes()).hexdigest() == e["input_sha256"]
    for per_level in ((False, True) if e["filter"] == "box" else (False,)):
        got = [_np(g, np.uint16) for g in itw.generate_mips(_dev(gpu, base), per_level=per_level)]
        assert hashlib.sha256(b"".join(np.ascontiguousarray(g).tobytes() for g in got[1:])).hexdigest() == e["levels_sha256"], (name, per_level)
        if e["stored"]:
            for i, g in enumerate(got[1:], 1):
                assert np.array_equal(g, gold[f"{name}_l{i}"]), (name, i)


LINEAR_SIZES = [(3, 1), (1, 3), (5, 3), (7, 7), (100, 36), (127, 339), (96, 64)]       # (width, height)


@pytest.mark.parametrize("kind", ["u8", "f16"])
@pytest.mark.parametrize("w,h", LINEAR_SIZES)
def test_linear_chains_of_two_items(itw, gpu, kind, w, h):
    import torch
    bases = [_content(kind, h, w, 31 * w + h + i) for i in range(2)]
    got = itw.generate_mips([_dev(gpu, b) for b in bases])
    flagged = itw.generate_mips([_dev(gpu, b) for b in bases], per_level=True)      # the flag changes nothing for a linear chain
    torch.cuda.synchronize()
    for i, b in enumerate(bases):
        want = M.chain(b)
        _equal_chain(got[i], want, (w, h, kind, "item", i))
        _equal_chain(flagged[i], want, (w, h, kind, "item", i, "flag"))
    host = itw.generate_mips(bases[0], levels=min(3, M.levels_of(w, h)))
    _equal_chain(host, M.chain(bases[0], len(host)), (w, h, kind, "host"))


def _canvas_chain(base, device, items):
    """Every level of every item a strided view inside ONE pattern-filled canvas, three pattern rows and a few pattern texels around each;
    the rows start 3 texels past a 16-byte boundary, so no vector access applies.  Returns (canvas, chains of views, first row of every
    view, the pattern)."""
    h, w = base.shape[:2]
    isz = base.itemsize
    n = M.levels_of(w, h)
    pitch = (3 + w + 5) * 4 * isz
    pitch += (-pitch) % 16
    rows = 3 + items * sum(max(1, h >> l) + 3 for l in range(n))
    pattern = G.pattern(rows * pitch).reshape(rows, pitch)
    if device is None:
        canvas = pattern.copy()
        texels = canvas.view(base.dtype)
    else:
        import torch
        canvas = torch.from_numpy(pattern.copy()).to(device)
        texels = canvas.view(torch.int16) if isz == 2 else canvas
    chains, tops, y = [], [], 3
    for _ in range(items):
        ch, top = [], []
        for l in range(n):
            lw, lh = M.level_size(w, h, l)
            sub = texels[y:y + lh, 12:(3 + lw) * 4]
            ch.append(np.lib.stride_tricks.as_strided(sub, (lh, lw, 4), (sub.strides[0], 4 * isz, isz)) if device is None else sub.unflatten(1, (lw, 4)))
            top.append(y)
            y += lh + 3
        chains.append(ch)
        tops.append(top)
    return canvas, chains, tops, pattern


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("kind", ["u8", "f16"])
@pytest.mark.parametrize("w,h", [(128, 128), (64, 32), (20, 12)])
def test_levels_as_views_of_one_canvas_and_nothing_else_is_written(itw, gpu, kind, w, h, where):
    """The canvas after the call is the pattern with the bases and the model's levels in their places, byte for byte: level 0 is not
    written, and neither is anything outside width x height of a written level."""
    import torch
    bases = [_content(kind, h, w, 900 + w + i) for i in range(2)]
    px = 4 * bases[0].itemsize
    for per_level in ((False, True) if M.is_pow2(w) else (False,)):
        canvas, chains, tops, pattern = _canvas_chain(bases[0], gpu if where == "device" else None, 2)
        expected = pattern.copy()
        for ch, top, b in zip(chains, tops, bases):
            if where == "device":
                ch[0].copy_(_dev(gpu, b))
                assert all(lv.data_ptr() % 16 != 0 for lv in ch)
            else:
                ch[0][...] = b
            for lv, y in zip(M.chain(b), top):
                expected[y:y + lv.shape[0], 3 * px:(3 + lv.shape[1]) * px] = lv.view(np.uint8).reshape(lv.shape[0], lv.shape[1] * px)
        itw.generate_mips_into(chains, per_level=per_level)
        torch.cuda.synchronize()
        after = canvas.cpu().numpy() if where == "device" else canvas
        bad = np.argwhere(after != expected)
        assert bad.size == 0, (w, h, kind, where, per_level, len(bad), bad[:4].tolist())


def test_mixed_pointer_kinds_are_refused(itw, gpu):
    base = _bytes(8, 8, 1)
    lv = np.zeros((4, 4, 4), np.uint8)
    itw.set_error_mode(itw.ON_ERROR_RETURN)
    try:
        with pytest.raises(ValueError, match="host or all device"):
            itw.generate_mips_into([[_dev(gpu, base), lv]])
        ok, out = itw.compress_mipped("bc1", [_dev(gpu, base), base.copy()], out=np.zeros(2 * 3 * 8 * 4, np.uint8))
        assert ok is False and "host or all device" in itw.last_error() and not out.any()
    finally:
        itw.lib().itwClearError()
        itw.set_error_mode(itw.ON_ERROR_ABORT)
    assert not lv.any()


def _settings(itw, fmt):
    return {"bc7": lambda: itw.bc7_profile("ultrafast"), "bc6h": lambda: itw.bc6h_profile("veryfast"), "etc1": lambda: itw.EtcSettings(1)}.get(fmt, lambda: None)()


def _shapes(fmt):
    kind = "f16" if fmt == "bc6h" else "u8"
    return {"20x12": [_content(kind, 12, 20, 3)], "64^2 cube": [_content(kind, 64, 64, 50 + f) for f in range(6)]}


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("fmt,ops", [("bc1", 0), ("bc7", 0), ("bc6h", 0), ("etc1", 0), ("bc5", 7)])
def test_mipped_is_generate_then_the_chain_call(itw, gpu, fmt, ops, where):
    import torch
    for name, bases in _shapes(fmt).items():
        src = [_dev(gpu, b) for b in bases] if where == "device" else [b.copy() for b in bases]
        ok, got = itw.compress_mipped(fmt, src, settings=_settings(itw, fmt), normal_ops=ops)
        torch.cuda.synchronize()
        assert ok, (name, itw.last_error())
        for s, b in zip(src, bases):
            assert np.array_equal(_np(s, b.dtype), b), "a base was written"
        # the composition a caller would write: flip level 0, generate, then the chain call (with the normalise in its gather)
        work = [_dev(gpu, b) for b in bases]
        if ops & 3:
            itw.prepare_normal_map(work, ops=ops & 3)
        chains = itw.generate_mips(work)
        flat = [lv for ch in chains for lv in ch]
        ok, want = itw.compress_chain(fmt, flat, settings=_settings(itw, fmt), normal_ops=(ops & 4) or None)
        torch.cuda.synchronize()
        assert ok and got.shape == want.shape and np.array_equal(_np(got, np.uint8), _np(want, np.uint8)), (fmt, name, where)


def test_mipped_bc5_keeps_the_reference_order_flip_mips_normalise(itw, gpu):
    """Against the model: flips on level 0, the mip filter, the normalise on every level.  Flipping AFTER the mips gives other bytes (255 - x
    does not commute with the store's round-half-up), so the order is pinned."""
    for w, h in ((20, 12), (64, 64)):
        base = _bytes(h, w, 77)
        ok, got = itw.compress_mipped("bc5", _dev(gpu, base), normal_ops=7)
        assert ok
        right = [N.prepare(lv, 4) for lv in M.chain(N.prepare(base, 3))]
        wrong = [N.prepare(lv, 7) for lv in M.chain(base)]
        assert any(not np.array_equal(a, b) for a, b in zip(right, wrong))
        want = itw.compress_chain("bc5", right)[1]
        other = itw.compress_chain("bc5", wrong)[1]
        assert np.array_equal(_np(got, np.uint8), want) and not np.array_equal(want, other), (w, h)


def test_mipped_bc1_against_the_cpu_oracle(itw, gpu, oracle):
    bases = [_bytes(64, 64, 60 + f) for f in range(6)]
    ok, got = itw.compress_mipped("bc1", bases)
    assert ok
    want = np.concatenate([oracle.encode("bc1", itw.pad_to_multiple_of_4(lv)).reshape(-1) for b in bases for lv in M.chain(b)])
    assert got.size == want.size and np.array_equal(got, want.view(np.uint8).reshape(-1))


def test_mipped_progress_and_the_early_out(itw, gpu):
    bases = [_dev(gpu, _bytes(64, 64, 80 + f)) for f in range(6)]
    n = 6 * 7
    ok, want = itw.compress_mipped("bc1", bases)
    calls = []
    ok, got = itw.compress_mipped("bc1", bases, progress=lambda i, t, u: calls.append((i, t)) or True)
    assert ok and calls == [(i, n) for i in range(1, n + 1)] and np.array_equal(_np(got, np.uint8), _np(want, np.uint8))
    k = 9
    calls = []

    def stop_at_k(i, t, u):
        calls.append(i)
        return i != k

    ok, got = itw.compress_mipped("bc1", bases, progress=stop_at_k)
    assert ok is False and calls == list(range(1, k + 1))
    ok, two = itw.compress_mipped("bc1", bases, levels=2)
    assert ok and two.numel() == 6 * (256 + 64) * 8
