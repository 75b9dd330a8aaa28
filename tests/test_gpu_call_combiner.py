"""The call combiner (csrc/abi.hip: coalesce_small_call, run_batch, continues, same_settings) decides which texels are encoded under which
settings into which bytes when several host threads call CompressBlocks* at once.  Here its decisions are pinned: every scenario holds its
N concurrent calls into ONE batch (itwTestCombinerHold of the hooks build), so what the leader merges no longer depends on arrival times,
and then asserts

* bytes: every request's destination equals the CPU oracle's encoding of that request alone, its own texels under its own settings, and
  nothing around the destinations changed (tests/_combiner.py);
* counters (itwTestCombinerCounters): N requests, one batch, no hold ended by its timeout, and exactly M merged calls -- M == 1 where the
  requests continue each other, M == N (or the stated number) where they only look as if they did.

Shapes are the smallest that can go wrong: bands of 4-12 texel rows of a 64-texel-wide image, about 256 blocks per scenario."""
import ctypes as C

import numpy as np
import pytest

import _combiner as cb
from _combiner import N, Scenario, run

pytestmark = pytest.mark.gpu

W = 64
BAND = 8
SIGNED = ("bc4_snorm", "bc5_snorm")


@pytest.fixture(scope="module")
def T(itw, gpu):
    """The hooks build: its combiner and counters are its own.  Errors return for the module's tests (each call's itwLastError is asserted)."""
    L = itw.test_lib()
    L.itwSetErrorMode(itw.ON_ERROR_RETURN)
    yield L
    L.itwSetErrorMode(itw.ON_ERROR_ABORT)


# ---- content -----------------------------------------------------------------------------------------------------------------

def ldr(w=W, rows=64):
    """ldr_smooth rows followed by ldr_uniform rows, twice over the height: neighbouring bands differ, and both halves hold both kinds."""
    from itw_amd import surfaces
    q = rows // 4
    sm, un = surfaces.ldr_smooth(2 * q, w), surfaces.ldr_uniform(2 * q, w)
    return np.ascontiguousarray(np.concatenate([sm[:q], un[:q], sm[q:], un[q:]], axis=0))


def hdr(w=W, rows=64):
    from itw_amd import surfaces
    return surfaces.hdr_smooth(rows, w)


def content(fmt, w=W, rows=64):
    if fmt == "bc6h":
        return hdr(w, rows)
    img = ldr(w, rows)
    return img.view(np.int8) if fmt in SIGNED else img


def settings_of(itw, fmt, prof=None):
    if fmt == "bc7":
        return itw.bc7_profile(prof or "basic")
    if fmt == "bc6h":
        return itw.bc6h_profile(prof or "fast")
    return None


def clone(s):
    return type(s).from_buffer_copy(bytes(s))


def changed(s, field, index, value):
    t = clone(s)
    if index is None:
        setattr(t, field, value)
    else:
        getattr(t, field)[index] = value
    assert bytes(t) != bytes(s), (field, index, value)
    return t


def check(d, n, calls):
    assert d["requests"] == n, d
    assert d["batches"] == 1, d
    assert d["hold_timeouts"] == 0, d
    if isinstance(calls, tuple):
        assert calls[0] <= d["calls"] <= calls[1], d
    else:
        assert d["calls"] == calls, d


def bands(sc, fmts, settings, src, heights):
    """Consecutive bands of `src`, consecutive destinations: request k is fmts[k % len] under settings[k % len]."""
    y = 0
    for k, h in enumerate(heights):
        sc.add(fmts[k % len(fmts)], settings[k % len(settings)], src, y, h)
        y += h
    return sc


# ---- scenarios that must merge ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["bc1", "bc3", "bc4", "bc5", "bc4_snorm", "bc5_snorm", "bc7", "bc6h"])
def test_consecutive_bands_with_one_settings_struct_are_one_call(itw, T, oracle, fmt):
    sc = Scenario(oracle)
    bands(sc, [fmt], [settings_of(itw, fmt)], sc.source(content(fmt)), [BAND] * N)
    check(run(itw, T, sc), N, 1)


def test_bands_of_unequal_heights_are_one_call(itw, T, oracle):
    sc = Scenario(oracle)
    heights = [4, 8, 12, 4, 8, 12, 8, 8]
    bands(sc, ["bc3"], [None], sc.source(ldr()), heights)
    assert sum(heights) == 64 and len(heights) == N
    check(run(itw, T, sc), N, 1)


def test_a_padded_pitch_is_one_call(itw, T, oracle):
    sc = Scenario(oracle)
    src = sc.source(ldr(), row_pad=64)
    assert src.stride == W * 4 + 64
    bands(sc, ["bc7"], [settings_of(itw, "bc7")], src, [BAND] * N)
    check(run(itw, T, sc), N, 1)


def test_width_70_with_a_tight_stride_is_one_call_of_17_block_columns(itw, T, oracle):
    """An ISPC format drops the partial block column: each band writes 17 blocks per block row and the oracle runs on the first 68 columns."""
    sc = Scenario(oracle)
    src = sc.source(ldr(72)[:, :70])
    assert src.stride == 70 * 4
    bands(sc, ["bc1"], [None], src, [BAND] * N)
    assert all(r.want.size == 2 * 17 * 8 for r in sc.reqs)
    check(run(itw, T, sc), N, 1)


def test_bc5_62_by_61_with_a_partial_last_band_is_one_call(itw, T, oracle):
    """Bands of 16, 16, 16 and 13 rows: four requests; the oracle encodes the whole image and each band owns its block rows of that stream."""
    img = np.ascontiguousarray(ldr()[:61, :62])
    whole = oracle.encode_bc45("bc5", img)
    assert whole.size == 16 * 16 * 16
    sc = Scenario(oracle)
    src = sc.source(img)
    y = 0
    for h in (16, 16, 16, 13):
        sc.add("bc5", None, src, y, h, want=whole[(y // 4) * 16 * 16:((y + h + 3) // 4) * 16 * 16].copy())
        y += h
    check(run(itw, T, sc), 4, 1)


# ---- settings: one field at a time ------------------------------------------------------------------------------------------
# (format, base preset, changes to the preset that make the field matter, field, index, value of struct B).  Bases and values were chosen
# on the CPU so that the oracle's output differs between A and B on this content; the tests assert it.
FIELDS = [
    ("bc7", "basic", {}, "mode_selection", 0, False),
    ("bc7", "alpha_basic", {}, "mode_selection", 1, False),
    ("bc7", "basic", {}, "mode_selection", 2, False),
    ("bc7", "alpha_ultrafast", {}, "mode_selection", 3, False),
    ("bc7", "basic", {}, "refineIterations", 0, 0),
    ("bc7", "veryfast", {}, "refineIterations", 1, 0),
    ("bc7", "slow", {}, "refineIterations", 2, 0),
    ("bc7", "veryfast", {"fastSkipTreshold_mode1": 0, "fastSkipTreshold_mode3": 16}, "refineIterations", 3, 0),      # (mode 3 wins only where mode 1 does not run)
    ("bc7", "basic", {}, "refineIterations", 4, 0),
    ("bc7", "alpha_ultrafast", {}, "refineIterations", 5, 5),
    ("bc7", "ultrafast", {}, "refineIterations", 6, 0),
    ("bc7", "basic", {}, "skip_mode2", None, False),
    ("bc7", "veryfast", {}, "fastSkipTreshold_mode1", None, 1),
    ("bc7", "veryfast", {"fastSkipTreshold_mode1": 0}, "fastSkipTreshold_mode3", None, 16),
    ("bc7", "alpha_basic", {}, "fastSkipTreshold_mode7", None, 0),
    ("bc7", "basic", {}, "mode45_channel0", None, 1),
    ("bc7", "alpha_basic", {}, "refineIterations_channel", None, 4),
    ("bc7", "basic", {}, "channels", None, 4),
    ("bc6h", "fast", {}, "slow_mode", None, True),
    ("bc6h", "fast", {}, "fast_mode", None, False),
    ("bc6h", "veryfast", {}, "refineIterations_1p", None, 1),
    ("bc6h", "fast", {}, "refineIterations_2p", None, 2),
    ("bc6h", "fast", {}, "fastSkipTreshold", None, 0),
]


def two_structs(itw, fmt, base, mods, field, index, value):
    a = settings_of(itw, fmt, base)
    for k, v in mods.items():
        setattr(a, k, v)
    return a, changed(a, field, index, value)


def settings_scenario(itw, oracle, fmt, a, b, layout):
    """Bands alternating A, B, A, B ... or A A A A B B B B.  Precondition: under B's place the oracle gives other bytes for A than for B in at
    least one band, so a merge across the settings -- which runs B's bands under the chain's first struct, A -- necessarily changes bytes."""
    img = content(fmt)
    who = [a, b] * 4 if layout == "alternating" else [a] * 4 + [b] * 4
    sc = Scenario(oracle)
    src = sc.source(img)
    differ = 0
    for k in range(N):
        sc.add(fmt, who[k], src, k * BAND, BAND)
        if who[k] is b:
            differ += not np.array_equal(cb.want_bytes(oracle, fmt, a, img[k * BAND:(k + 1) * BAND]), sc.reqs[-1].want)
    assert differ >= 1, "precondition: structs A and B encode none of B's bands differently"
    return sc


@pytest.mark.parametrize("layout,calls", [("alternating", 8), ("halves", 2)])
@pytest.mark.parametrize("fmt,base,mods,field,index,value", FIELDS, ids=[f"{f[0]}-{f[3]}{'' if f[4] is None else f[4]}" for f in FIELDS])
def test_structs_that_differ_in_one_field_are_not_merged(itw, T, oracle, fmt, base, mods, field, index, value, layout, calls):
    a, b = two_structs(itw, fmt, base, mods, field, index, value)
    check(run(itw, T, settings_scenario(itw, oracle, fmt, a, b, layout)), N, calls)


def test_refine_iterations_7_is_ignored_where_mode_7_does_not_run(itw, T, oracle):
    """An RGB preset never writes refineIterations[7] and, with fastSkipTreshold_mode7 == 0, the encoder never reads it: eight structs that differ
    only there are one call, and each band still equals the oracle under its OWN struct."""
    base = settings_of(itw, "bc7", "basic")
    assert base.fastSkipTreshold_mode7 == 0
    structs = [changed(base, "refineIterations", 7, v) for v in (1, 2, 3, 4, 5, 77, -3, 1 << 20)]
    sc = Scenario(oracle)
    bands(sc, ["bc7"], structs, sc.source(ldr()), [BAND] * N)
    check(run(itw, T, sc), N, 1)


def test_refine_iterations_7_separates_calls_where_mode_7_runs(itw, T, oracle):
    a, b = two_structs(itw, "bc7", "alpha_basic", {}, "refineIterations", 7, 0)
    assert a.fastSkipTreshold_mode7 > 0 and a.mode_selection[1]
    check(run(itw, T, settings_scenario(itw, oracle, "bc7", a, b, "alternating")), N, 8)


# ---- formats of one block and texel size in turn ---------------------------------------------------------------------------------

@pytest.mark.parametrize("fmts", [("bc3", "bc7", "bc5", "bc5_snorm"), ("bc1", "bc4", "bc4_snorm")], ids=["16-byte-blocks", "8-byte-blocks"])
def test_formats_in_turn_on_consecutive_bands_are_not_merged(itw, T, oracle, fmts):
    sc = Scenario(oracle)
    bands(sc, list(fmts), [settings_of(itw, f) for f in fmts], sc.source(ldr()), [BAND] * N)
    assert len({r.want.size for r in sc.reqs}) == 1               # same block size: the destinations continue each other exactly
    check(run(itw, T, sc), N, 8)


# ---- geometry ----------------------------------------------------------------------------------------------------------------

def test_ispc_bands_of_10_rows_are_not_merged(itw, T, oracle):
    """Each band encodes its own first 8 rows into 2 block rows; the destinations are 10 / 4 = 2 block rows apart, the sources 10 rows: merged, the
    second band's block rows would come from rows 8-15 of the first."""
    sc = Scenario(oracle)
    bands(sc, ["bc3"], [None], sc.source(ldr(rows=80)), [10] * N)
    assert all(r.want.size == 2 * 16 * 16 for r in sc.reqs)
    check(run(itw, T, sc), N, 8)


def test_bc4_bands_with_a_partial_third_block_row_are_not_merged(itw, T, oracle):
    sc = Scenario(oracle)
    bands(sc, ["bc4"], [None], sc.source(ldr(rows=80)), [10] * N)
    assert all(r.want.size == 3 * 16 * 8 for r in sc.reqs)
    check(run(itw, T, sc), N, 8)


def test_left_and_right_halves_are_two_calls(itw, T, oracle):
    """Width 32 of a 64-wide image at the image's stride, four bands each: in address order the two halves' bands alternate."""
    sc = Scenario(oracle)
    src = sc.source(ldr(rows=32))
    for x0 in (0, 32):
        for k in range(4):
            sc.add("bc7", settings_of(itw, "bc7"), src, k * BAND, BAND, x0=x0, w=32)
    check(run(itw, T, sc), N, 2)


@pytest.mark.parametrize("order", ["gap", "reverse"])
def test_destinations_that_do_not_continue_are_not_merged(itw, T, oracle, order):
    """Consecutive source bands; destinations one block row too far apart, or in reverse order."""
    sc = Scenario(oracle)
    src = sc.source(ldr())
    size = 2 * 16 * 16
    for k in range(N):
        sc.add("bc3", None, src, k * BAND, BAND, dst=k * (size + 16 * 16) if order == "gap" else (N - 1 - k) * size)
    check(run(itw, T, sc), N, 8)


def test_every_other_source_band_with_consecutive_destinations_is_not_merged(itw, T, oracle):
    sc = Scenario(oracle)
    src = sc.source(ldr(rows=128))
    for k in range(N):
        sc.add("bc3", None, src, 2 * k * BAND, BAND)
    check(run(itw, T, sc), N, 8)


def test_a_band_that_starts_where_the_last_ends_with_another_stride_is_not_merged(itw, T, oracle):
    """Four pairs carved from one byte buffer: band A at stride 256, band B exactly at A.ptr + A.height * A.stride with stride 320, both 64 wide;
    destinations consecutive.  Two calls per pair."""
    img = ldr(rows=128)
    row = W * 4
    pair = BAND * row + BAND * (row + 64) + 192                    # (+ 192: the next pair does not start where this one ends)
    buf = np.full(4 * pair, 0x5a, dtype=np.uint8)
    for p in range(4):
        a, b = buf[p * pair:p * pair + BAND * row], buf[p * pair + BAND * row:p * pair + BAND * row + BAND * (row + 64)]
        a.reshape(BAND, row)[:] = img[2 * p * BAND:(2 * p + 1) * BAND].reshape(BAND, row)
        b.reshape(BAND, row + 64)[:, :row] = img[(2 * p + 1) * BAND:(2 * p + 2) * BAND].reshape(BAND, row)
    sc = Scenario(oracle)
    src = sc.raw(buf)
    for p in range(4):
        sc.add_raw("bc3", None, src.ptr + p * pair, W, BAND, row, img[2 * p * BAND:(2 * p + 1) * BAND])
        sc.add_raw("bc3", None, src.ptr + p * pair + BAND * row, W, BAND, row + 64, img[(2 * p + 1) * BAND:(2 * p + 2) * BAND])
    for a, b in zip(sc.reqs[0::2], sc.reqs[1::2]):
        assert b.ptr == a.ptr + a.height * a.stride and b.stride != a.stride and b.dst_off == a.dst_off + a.want.size
    check(run(itw, T, sc), N, 8)


def test_bottom_up_bands_are_never_merged(itw, T, oracle):
    """Negative stride: band k starts at the last row of its rows and reads upwards; each next band starts at ptr + height * stride of the last."""
    img = ldr()
    sc = Scenario(oracle)
    src = sc.source(img)
    for k in range(N):
        top = 64 - (k + 1) * BAND
        sc.add_raw("bc3", None, src.ptr + (top + BAND - 1) * src.stride, W, BAND, -src.stride, img[top:top + BAND][::-1])
    for a, b in zip(sc.reqs, sc.reqs[1:]):
        assert b.ptr == a.ptr + a.height * a.stride
    check(run(itw, T, sc), N, 8)


def test_bands_of_stride_0_are_never_merged(itw, T, oracle):
    """Stride 0 repeats one row; ptr + height * stride is the band's own pointer, so requests of the same row `continue` each other."""
    img = ldr()
    sc = Scenario(oracle)
    src = sc.source(img)
    for k in range(N):
        r = 4 * (k // 2)
        sc.add_raw("bc3", None, src.ptr + r * src.stride, W, BAND, 0, np.repeat(img[r:r + 1], BAND, axis=0))
    check(run(itw, T, sc), N, 8)


def test_four_source_bands_to_two_destinations(itw, T, oracle):
    """Eight threads, two per source band.  The sort's order among equal pointers is not fixed: between 2 and 8 calls."""
    sc = Scenario(oracle)
    src = sc.source(ldr(rows=32))
    for copy in range(2):
        for k in range(4):
            sc.add("bc7", settings_of(itw, "bc7"), src, k * BAND, BAND)
    check(run(itw, T, sc), N, (2, 8))


# ---- bytes only --------------------------------------------------------------------------------------------------------------

def random_bc7_struct(itw, rng):
    """tests/test_gpu_parity_bc7.py test_random_settings_fuzz's generator and ranges."""
    thresholds = [0, 1, 2, 5, 12, 16, 17, 40, 63, 64, 70]
    s = itw.Bc7Settings()
    s.skip_mode2 = bool(rng.integers(0, 2))
    s.fastSkipTreshold_mode1 = int(rng.choice(thresholds))
    s.fastSkipTreshold_mode3 = int(rng.choice(thresholds))
    s.fastSkipTreshold_mode7 = int(rng.choice(thresholds))
    s.mode45_channel0 = int(rng.integers(0, 4))
    s.refineIterations_channel = int(rng.integers(0, 6))
    s.channels = int(rng.choice([3, 4]))
    sel = [bool(rng.integers(0, 2)) for _ in range(4)]
    if not any(sel):
        sel[int(rng.integers(0, 4))] = True
    for i in range(4):
        s.mode_selection[i] = sel[i]
    for i in range(8):
        s.refineIterations[i] = int(rng.integers(0, 6))
    return s


def random_bc6h_struct(itw, rng):
    """tests/test_gpu_bc7_paths.py test_bc6h_random_settings_on_each_shape's generator and ranges."""
    s = itw.Bc6hSettings()
    s.slow_mode = bool(rng.integers(0, 2))
    s.fast_mode = bool(rng.integers(0, 2))
    s.refineIterations_1p = int(rng.integers(0, 4))
    s.refineIterations_2p = int(rng.integers(0, 4))
    s.fastSkipTreshold = int(rng.choice([0, 1, 2, 3, 8, 10, 31, 32, 33, 64]))
    return s


@pytest.mark.parametrize("fmt", ["bc7", "bc6h"])
def test_random_structs_from_a_pool_of_three(itw, T, oracle, fmt):
    """Whatever merges, each band equals the oracle under its own struct."""
    rng = np.random.default_rng(20261018 + (6 if fmt == "bc6h" else 7))
    for rnd in range(3):
        pool = [(random_bc7_struct if fmt == "bc7" else random_bc6h_struct)(itw, rng) for _ in range(3)]
        sc = Scenario(oracle)
        src = sc.source(content(fmt))
        for k in range(N):
            sc.add(fmt, pool[int(rng.integers(0, 3))], src, k * BAND, BAND)
        d = run(itw, T, sc)
        assert d["requests"] == N, (rnd, d)


@pytest.mark.parametrize("fmt,prof", [("bc7", "basic"), ("bc6h", "slow")])
def test_leadership_handed_over_within_a_burst(itw, T, oracle, fmt, prof):
    """The hold asks for half the threads, so the burst ends as two or more batches led by different threads in the device's one shared context;
    the widths grow from round to round, so a later leader regrows the staging buffers and the workspace an earlier one created."""
    for w in (64, 256, 1024):
        img = content(fmt, w, rows=32)
        st = settings_of(itw, fmt, prof)
        whole = oracle.encode_mt(fmt, img, oracle.Bc7Settings.from_buffer_copy(bytes(st)) if fmt == "bc7" else oracle.Bc6hSettings.from_buffer_copy(bytes(st)),
                                 threads=8).reshape(-1)
        per = (w // 4) * 16
        sc = Scenario(oracle)
        src = sc.source(img)
        for k in range(N):
            sc.add(fmt, st, src, 4 * k, 4, want=whole[k * per:(k + 1) * per].copy())
        d = run(itw, T, sc, hold=N // 2)
        assert d["requests"] == N, (w, d)


def test_a_ninth_thread_on_the_device_resident_path(itw, T, gpu, oracle):
    """While eight host callers burst, a ninth thread makes device-resident bc7 calls on a stream of its own (itwSetStream): those never enter
    the combiner, and both kinds of call give the oracle's bytes."""
    import torch
    st = settings_of(itw, "bc7")
    img = ldr()
    sc = Scenario(oracle)
    bands(sc, ["bc7"], [st], sc.source(img), [BAND] * N)
    other = np.ascontiguousarray(img[::-1])
    want = cb.want_bytes(oracle, "bc7", st, other)
    d_img = torch.from_numpy(other).to(gpu)
    rounds = 6
    d_out = torch.zeros((rounds, want.size), dtype=torch.uint8, device=gpu)
    stream = torch.cuda.Stream(device=gpu)
    torch.cuda.synchronize()
    err = []

    def resident():
        T.itwSetStream(C.c_void_p(stream.cuda_stream))
        surf = itw.RgbaSurface(d_img.data_ptr(), W, 64, W * 4)
        for r in range(rounds):
            T.CompressBlocksBC7(C.byref(surf), C.c_void_p(d_out[r].data_ptr()), C.byref(st))
            err.append(T.itwLastError())
        stream.synchronize()
        T.itwSetStream(None)

    d = run(itw, T, sc, extra=resident)
    assert d["requests"] == N, d
    assert err == [None] * rounds, err
    got = d_out.cpu().numpy()
    for r in range(rounds):
        assert np.array_equal(got[r], want), r
