"""The mip rules for cut-out textures on the device (include/itw_dispatch.h, "Mip chains of cut-out textures"; csrc/mip_alpha.hip):
alpha-weighted colour and coverage kept per level against the numpy model of tests/_alpha_mips.py, on both routes, from host and device
pointers, inside guarded canvases; the report; itwAlphaCoverage; the one-call save.  Every comparison is == on bytes or integers.  Every
test here fails on a build without the three entry points."""
import ctypes as C
import functools

import numpy as np
import pytest

import _alpha_mips as A
import _guarded as G
import _mipgen as M

pytestmark = pytest.mark.gpu

REFS = (1, 128, 255)
# (width, height, items): 128^2 and 256 x 64: a pyramid launch with register and LDS levels, then the tail; 64^2: one tile; 512 x 2: the
# per-level bridge; 32 x 8, 16 x 1, 1 x 16: the tail alone; the rest: the linear filter; six faces of 64^2, each with its own coverage;
# 512 x 256: a coverage workgroup walks 16 384 texels, so levels 0 and 1 take several workgroups each
BOX_CASES = [(128, 128, 1), (256, 64, 1), (64, 64, 1), (512, 2, 1), (32, 8, 1), (16, 1, 1), (1, 16, 1), (64, 64, 6), (512, 256, 1)]
LINEAR_CASES = [(130, 66, 1), (37, 19, 1), (5, 3, 1), (1, 7, 1), (37, 19, 6)]


def _dev(gpu, a):
    import torch
    return torch.from_numpy(np.array(a)).to(gpu)                  # (a copy: the shared bases are read-only)


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


@functools.lru_cache(maxsize=None)
def _bases(w, h, items, content):
    """content "cutout": alpha spiked at 0 and 255 with soft edges, arbitrary colour under alpha 0, the left half transparent; "noise":
    uniform alpha.  Of six items face 1 is fully transparent and face 2 fully opaque, whatever the content."""
    out = []
    for i in range(items):
        seed = 7000 + 97 * w + 13 * h + i
        img = A.cutout(h, w, seed, hole=(i % 2 == 0)) if content == "cutout" else A.noise(h, w, seed)
        if items == 6 and i == 1:
            img[..., 3] = 0
        if items == 6 and i == 2:
            img[..., 3] = 255
        img.setflags(write=False)
        out.append(img)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _model(w, h, items, content, srgb, weight, ref):
    """Per item (levels, rows or None): computed once, shared, never written."""
    out = []
    for b in _bases(w, h, items, content):
        levels, rows = A.chain(b, srgb=srgb, weight=weight, ref=ref)
        for lv in levels:
            lv.setflags(write=False)
        out.append((tuple(levels), rows))
    return tuple(out)


def _rows(report):
    return [(int(r.texels), int(r.covered_plain), int(r.covered), int(r.threshold)) for r in report]


def _check_chain(itw, gpu, w, h, items, content, srgb, weight, ref, where="device"):
    """Both routes against the model, the report included where there is one."""
    import torch
    want = _model(w, h, items, content, srgb, weight, ref)
    for per_level in (False, True):
        src = [_dev(gpu, b) if where == "device" else b.copy() for b in _bases(w, h, items, content)]
        got = itw.generate_mips(src, per_level=per_level, srgb=srgb, alpha_weight=weight, alpha_coverage=ref, report=bool(ref))
        torch.cuda.synchronize()
        chains, report = got if ref else (got, None)
        for i, (ch, (levels, rows)) in enumerate(zip(chains, want)):
            for l, (g, lv) in enumerate(zip(ch, levels)):
                bad = np.argwhere(_np(g) != lv)
                assert bad.size == 0, (w, h, content, srgb, weight, ref, per_level, where, i, l, len(bad), bad[:3].tolist())
        if ref:
            assert _rows(report) == [row for _, rows in want for row in rows], (w, h, content, srgb, weight, ref, per_level)


def _invisible_levels(w, h, items, content):
    """The levels (>= 1) of item 0's weighted chain that hold an output texel with va == 0."""
    levels = _model(w, h, items, content, False, True, 0)[0][0]
    linear = not (M.is_pow2(w) and M.is_pow2(h))
    return {l for l in range(1, len(levels)) if A.invisible_mask(levels[l - 1], linear).any()}


def test_the_expected_chains_hold_the_cases_they_are_there_for():
    """No device: what the comparisons below would show nothing without."""
    assert {1, 2} <= _invisible_levels(128, 128, 1, "cutout")                  # the pyramid kernel's register levels
    assert {3, 4, 5, 6} <= _invisible_levels(128, 128, 1, "cutout")            # its LDS levels
    assert {1, 2, 3, 4, 5, 6} <= _invisible_levels(256, 64, 1, "cutout")
    assert {1, 2} <= _invisible_levels(32, 8, 1, "cutout") and _invisible_levels(1, 16, 1, "cutout")      # the tail kernel
    assert {1, 2, 3} <= _invisible_levels(512, 2, 1, "cutout")                 # the per-level kernel, box
    assert _invisible_levels(130, 66, 1, "cutout") and _invisible_levels(5, 3, 1, "cutout")               # and linear
    for content in ("cutout", "noise"):                                        # weighting changes bytes, and only colour
        a, b = _model(128, 128, 1, content, False, True, 0)[0][0], _model(128, 128, 1, content, False, False, 0)[0][0]
        assert not np.array_equal(a[1][..., :3], b[1][..., :3]) and np.array_equal(a[1][..., 3], b[1][..., 3])
    below = above = same = clamped = 0
    for w, h, items in BOX_CASES + LINEAR_CASES:
        for content in ("cutout", "noise"):
            plain = _model(w, h, items, content, False, True, 0)
            for (levels, rows), (before, _) in zip(_model(w, h, items, content, False, True, 128), plain):
                for lv, pl, row in zip(levels[1:], before[1:], rows[1:]):
                    below += row[3] < 128
                    above += row[3] > 128
                    same += row[3] == 128
                    clamped += bool(((lv[..., 3] == 255) & (pl[..., 3] < 255)).any())
                    if row[3] == 128:
                        assert np.array_equal(lv, pl)
    assert below and above and same and clamped, (below, above, same, clamped)
    rows = _model(64, 64, 6, "cutout", False, True, 128)
    assert rows[1][1][0][1] == 0 and rows[2][1][0][1] == 64 * 64               # the transparent and the opaque face: cov0 = 0 and N0
    assert all(r[2] == 0 for r in rows[1][1]) and all(r[2] == r[0] for r in rows[2][1])
    assert len({rows[i][1][0][1] for i in range(6)}) >= 5                      # each face has its own coverage


@pytest.mark.parametrize("content", ["cutout", "noise"])
@pytest.mark.parametrize("w,h,items", BOX_CASES + LINEAR_CASES)
def test_chains_are_the_models_on_both_routes(itw, gpu, w, h, items, content):
    """weight x coverage (off, 1, 128, 255) x sRGB, all but the plain corner; device pointers."""
    for srgb in (False, True):
        for weight in (False, True):
            for ref in (0,) + REFS:
                if weight or ref:
                    _check_chain(itw, gpu, w, h, items, content, srgb, weight, ref)


@pytest.mark.parametrize("w,h,items", [(128, 128, 1), (512, 2, 1), (32, 8, 1), (130, 66, 1), (64, 64, 6)])
def test_host_pointers_give_the_same(itw, gpu, w, h, items):
    _check_chain(itw, gpu, w, h, items, "cutout", True, True, 128, where="host")
    _check_chain(itw, gpu, w, h, items, "noise", False, False, 255, where="host")
    _check_chain(itw, gpu, w, h, items, "cutout", False, True, 0, where="host")


def _canvas_chain(w, h, items, device):
    """Every level of every item a strided view inside ONE pattern-filled canvas, three pattern rows and a few pattern texels around each;
    rows start 3 texels past a 16-byte boundary.  Returns (canvas, chains of views, first row of every view, the pattern)."""
    n = M.levels_of(w, h)
    pitch = (3 + w + 5) * 4
    pitch += (-pitch) % 16
    rows = 3 + items * sum(max(1, h >> l) + 3 for l in range(n))
    pattern = G.pattern(rows * pitch).reshape(rows, pitch)
    if device is None:
        canvas = pattern.copy()
    else:
        import torch
        canvas = torch.from_numpy(pattern.copy()).to(device)
    chains, tops, y = [], [], 3
    for _ in range(items):
        ch, top = [], []
        for l in range(n):
            lw, lh = M.level_size(w, h, l)
            sub = canvas[y:y + lh, 12:(3 + lw) * 4]
            ch.append(np.lib.stride_tricks.as_strided(sub, (lh, lw, 4), (sub.strides[0], 4, 1)) if device is None else sub.unflatten(1, (lw, 4)))
            top.append(y)
            y += lh + 3
        chains.append(ch)
        tops.append(top)
    return canvas, chains, tops, pattern


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("w,h,items", [(128, 128, 1), (256, 64, 1), (512, 2, 1), (1, 16, 1), (130, 66, 1), (5, 3, 1), (64, 64, 6), (512, 256, 1)])
def test_strided_views_inside_a_guarded_canvas(itw, gpu, w, h, items, where):
    """The canvas after the call is the pattern with the bases and the model's levels in their places, byte for byte: no guard byte and no
    base byte changes, on either route, with both rules on."""
    import torch
    for srgb, ref, per_level in ((False, 128, False), (True, 255, True), (True, 1, False)):
        bases, want = _bases(w, h, items, "cutout"), _model(w, h, items, "cutout", srgb, True, ref)
        canvas, chains, tops, pattern = _canvas_chain(w, h, items, gpu if where == "device" else None)
        expected = pattern.copy()
        for ch, top, b, (levels, _) in zip(chains, tops, bases, want):
            if where == "device":
                ch[0].copy_(_dev(gpu, b))
            else:
                ch[0][...] = b
            for lv, y in zip(levels, top):
                expected[y:y + lv.shape[0], 12:(3 + lv.shape[1]) * 4] = lv.reshape(lv.shape[0], lv.shape[1] * 4)
        _, report = itw.generate_mips_into(chains, per_level=per_level, srgb=srgb, alpha_weight=True, alpha_coverage=ref, report=True)
        torch.cuda.synchronize()
        bad = np.argwhere(_np(canvas) != expected)
        assert bad.size == 0, (w, h, items, where, srgb, ref, per_level, len(bad), bad[:4].tolist())
        assert _rows(report) == [row for _, rows in want for row in rows]


def _raw_generate(L, itw, chains, flags, opts, want_report):
    import torch
    flat = [lv for ch in chains for lv in ch]
    L.itwSetStream(torch.cuda.current_stream(flat[0].device).cuda_stream)
    rows = (itw.MipCoverage * len(flat))() if want_report else None
    rc = L.itwGenerateMipChainAlpha(C.cast(itw.abi._surfaces(flat), C.c_void_p), len(chains), len(chains[0]), flags,
                                    C.cast(C.byref(opts), C.c_void_p) if opts is not None else None, C.cast(rows, C.c_void_p) if want_report else None)
    torch.cuda.synchronize()
    return rc, rows


def _empty_chain(gpu, b):
    import torch
    h, w = b.shape[:2]
    return [_dev(gpu, b)] + [torch.zeros((max(1, h >> l), max(1, w >> l), 4), dtype=torch.uint8, device=gpu) for l in range(1, M.levels_of(w, h))]


@pytest.mark.parametrize("w,h", [(128, 128), (37, 19), (512, 2)])
def test_with_the_options_off_the_bytes_are_the_plain_calls(itw, gpu, w, h):
    import torch
    L = itw.lib()
    for flags in (0, itw.MIP_SRGB, itw.MIP_PER_LEVEL | itw.MIP_SRGB):
        b = _bases(w, h, 1, "cutout")[0]
        plain = itw.generate_mips(_dev(gpu, b), per_level=bool(flags & 1), srgb=bool(flags & 4))
        torch.cuda.synchronize()
        for opts in (None, itw.MipAlpha(0, 0)):
            ch = _empty_chain(gpu, b)
            rc, _ = _raw_generate(L, itw, [ch], flags, opts, False)
            assert rc == 0, itw.last_error()
            assert all(np.array_equal(_np(g), _np(p)) for g, p in zip(ch, plain)), (w, h, flags, opts is None)


@pytest.mark.parametrize("ref", REFS)
def test_a_tie_is_decided_by_the_distance_to_the_reference(itw, gpu, ref):
    """A constructed alpha plane: level 1 holds 0 and 255 only (each 2 x 2 of the base is constant), so ge[t] is one number for t = 1 .. 255,
    every t misses K alike and the nearest to r wins: t* == r and the level keeps its bytes, whatever K asks for.  (The third key, the
    smaller t, cannot decide: ge is non-increasing, so where r - d and r + d miss alike r itself misses no more -- tests/test_alpha_mips_cpu.py.)"""
    import torch
    rng = np.random.default_rng(40 + ref)
    plane = np.where(rng.random((8, 8)) < 0.3, 255, 0).astype(np.uint8)
    base = rng.integers(0, 256, (16, 16, 4), dtype=np.uint8)
    base[..., 3] = np.repeat(np.repeat(plane, 2, axis=0), 2, axis=1)
    levels, rows = A.chain(base, ref=ref)
    assert set(np.unique(levels[1][..., 3])) == {0, 255} and rows[1][3] == ref and len(set(np.unique(levels[2][..., 3]))) > 2
    hist = A.histogram(np.where(plane == 255, 255, 0))
    assert len({A.ge_counts(hist)[t] for t in range(1, 256)}) == 1 and all(A.threshold(hist, k, ref) == ref for k in (0, 5, 64))
    got, report = itw.generate_mips(_dev(gpu, base), alpha_coverage=ref, report=True)
    torch.cuda.synchronize()
    assert all(np.array_equal(_np(g), lv) for g, lv in zip(got, levels)) and _rows(report) == rows


def test_both_histogram_kernels_count_alike(itw, gpu):
    """The hooks build can launch the histogram kernel that counts the 0 and 255 bins per wave in place of the product's (one LDS atomic per texel):
    the same chain, report and counts from both, on both contents."""
    T = itw.test_lib()
    try:
        for spikes in (0, 1):
            T.itwTestAlphaHistVariant(spikes)
            for content in ("cutout", "noise"):
                for w, h in ((128, 128), (37, 19)):
                    b = _bases(w, h, 1, content)[0]
                    levels, rows = _model(w, h, 1, content, False, True, 128)[0]
                    ch = _empty_chain(gpu, b)
                    rc, report = _raw_generate(T, itw, [ch], 0, itw.MipAlpha(1, 128), True)
                    assert rc == 0 and _rows(report) == rows, (spikes, content, w, h)
                    assert all(np.array_equal(_np(g), lv) for g, lv in zip(ch, levels)), (spikes, content, w, h)
                    out = (C.c_uint64 * 1)()
                    assert T.itwAlphaCoverage(C.cast(itw.abi._surfaces([ch[0]]), C.c_void_p), 1, 255, C.cast(out, C.c_void_p)) == 0
                    assert int(out[0]) == int(np.count_nonzero(b[..., 3] >= 255))
    finally:
        T.itwTestAlphaHistVariant(0)


@pytest.mark.parametrize("where", ["device", "host"])
def test_alpha_coverage_counts(itw, gpu, where):
    """1 x 1, 3 x 5, 64 x 64, 130 x 66 and 301 x 200 (several workgroups) in one call and alone, both contents, a strided view among them."""
    imgs = [A.noise(1, 1, 1), A.cutout(5, 3, 2), A.cutout(64, 64, 3), A.noise(66, 130, 4), A.cutout(66, 130, 5, hole=False), A.noise(200, 301, 8)]
    wide = A.noise(40, 96, 6)
    for ref in (0, 1, 128, 255):
        want = [int(np.count_nonzero(i[..., 3] >= ref)) for i in imgs] + [int(np.count_nonzero(wide[3:36, 5:70, 3] >= ref))]
        if where == "device":
            src = [_dev(gpu, i) for i in imgs] + [_dev(gpu, wide)[3:36, 5:70]]
        else:
            src = [i.copy() for i in imgs] + [wide[3:36, 5:70]]
        assert itw.alpha_coverage(src, ref) == want, ref
        assert [itw.alpha_coverage(s, ref) for s in src] == want, ref
    assert all(np.array_equal(_np(s), i) for s, i in zip(src, imgs))


def _mipped_alpha(itw, fmt, bases, flags, opts, settings):
    """itwCompressImageMippedAlpha as a caller writes it, from host bases: (ok, blocks)."""
    import torch
    h, w = bases[0].shape[:2]
    n = itw.mip_levels(w, h)
    nbytes = len(bases) * sum(((max(1, w >> l) + 3) // 4) * ((max(1, h >> l) + 3) // 4) for l in range(n)) * itw.BYTES_PER_BLOCK[fmt]
    out = np.zeros(nbytes, dtype=np.uint8)
    sp = C.cast(C.byref(settings), C.c_void_p) if settings is not None else None
    ok = itw.lib().itwCompressImageMippedAlpha(C.cast(itw.abi._surfaces(bases), C.c_void_p), len(bases), 0, flags,
                                               C.cast(C.byref(opts), C.c_void_p) if opts is not None else None, out.ctypes.data, itw.DXGI_FORMAT[fmt], sp, None, None)
    torch.cuda.synchronize()
    return bool(ok), out


@pytest.mark.parametrize("fmt", ["bc3", "bc7"])
@pytest.mark.parametrize("shape", ["64^2 cube", "37x19"])
def test_the_one_call_save_is_generate_then_the_chain_call(itw, gpu, fmt, shape):
    import torch
    w, h, items = (64, 64, 6) if shape.startswith("64") else (37, 19, 1)
    settings = itw.bc7_profile("ultrafast") if fmt == "bc7" else None
    bases = [b.copy() for b in _bases(w, h, items, "cutout")]
    for flags in (0, itw.MIP_SRGB):
        ok, got = _mipped_alpha(itw, fmt, bases, flags, itw.MipAlpha(1, 128), settings)
        assert ok, itw.last_error()
        chains = itw.generate_mips([_dev(gpu, b) for b in bases], srgb=bool(flags), alpha_weight=True, alpha_coverage=128)
        for ch, (levels, _) in zip(chains, _model(w, h, items, "cutout", bool(flags), True, 128)):
            assert all(np.array_equal(_np(g), lv) for g, lv in zip(ch, levels))
        ok, want = itw.compress_chain(fmt, [lv for ch in chains for lv in ch], settings=settings)
        torch.cuda.synchronize()
        assert ok and np.array_equal(got, _np(want)), (fmt, shape, flags)
        ok, bound = itw.compress_mipped(fmt, bases, settings=settings, srgb=bool(flags), alpha_weight=True, alpha_coverage=128)
        assert ok and np.array_equal(_np(bound), got)
        # options off: itwCompressImageMippedEx's payload, which is another
        ok, plain = itw.compress_mipped(fmt, bases, settings=settings, srgb=bool(flags))
        for opts in (None, itw.MipAlpha(0, 0)):
            ok2, off = _mipped_alpha(itw, fmt, bases, flags, opts, settings)
            assert ok and ok2 and np.array_equal(off, _np(plain)), (fmt, shape, flags)
        assert not np.array_equal(_np(plain), got)
    assert all(np.array_equal(b, o) for b, o in zip(bases, _bases(w, h, items, "cutout"))), "a base was written"
