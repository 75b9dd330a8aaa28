"""ETC1 through the chain call, the slice pipeline and a KTX file (include/itw_dispatch.h, the itwKtx* functions of include/itw_dds.h).

Expected bytes come from the golden streams (tests/golden/golden_etc1.npz: a surface tiled from a 64 x 64 golden input encodes to the tiled
golden blocks) or from the live reference library on the edge-replicated image (tests/_etc1.py: a missing library fails).  Chains too
large for the scalar reference compare against this library's own per-image pad + itwCompressBlocksETC1, as tests/test_gpu_chain.py
does.  Every comparison is ==.  The golden streams of neighbouring thresholds differ in 27 to 198 of their 256 blocks, so a call that
loses its threshold on the way down fails."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _etc1
from _guarded import guarded
from conftest import first_mismatch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = (1, 6, 32, 166)                      # 166: above the last split, treated as 165


def _golden_threshold(t):
    return min(t, 165)


@pytest.fixture(scope="module")
def golden():
    g = _etc1.load_golden()
    for v in g.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return g


@pytest.fixture
def slice_window(itw):
    yield itw.lib().itwSetSliceWindow
    itw.lib().itwSetSliceWindow(0)


def _tiled(golden, name, ty, tx):
    """A (64 ty) x (64 tx) surface tiled from the golden input `name`."""
    return np.ascontiguousarray(np.tile(golden[name], (ty, tx, 1)))


def _tiled_stream(golden, name, t, ty, tx):
    """... and the stream it encodes to: the golden blocks, tiled."""
    blocks = golden[f"{name}.t{_golden_threshold(t)}"].reshape(16, 16, 8)
    return np.tile(blocks, (ty, tx, 1)).reshape(-1)


def _pad(img):
    h, w = img.shape[:2]
    return np.ascontiguousarray(np.pad(img, ((0, -h % 4), (0, -w % 4), (0, 0)), mode="edge"))


_ref_cache = {}


def _ref_chain(levels, t, key):
    """The live reference on every edge-replicated image, concatenated; computed once per (key, threshold)."""
    _etc1.live_reference()
    if (key, t) not in _ref_cache:
        out = np.concatenate([_etc1.ref_encode(_pad(lv), _golden_threshold(t)) for lv in levels])
        out.setflags(write=False)
        _ref_cache[(key, t)] = out
    return _ref_cache[(key, t)]


def _loop(itw, levels, st):
    """This library's own per-image loop: pad, then itwCompressBlocksETC1."""
    return np.concatenate([itw.compress_numpy("etc1", itw.pad_to_multiple_of_4(lv), st) for lv in levels])


def _host(out):
    return out.cpu().numpy() if hasattr(out, "cpu") else np.asarray(out)


def _same(got, want, what):
    got = _host(got)
    assert got.size == want.size, (what, got.size, want.size)
    m = first_mismatch(got, want, 8)
    assert m is None, (what, m)


def _device(gpu, img):
    import torch
    return torch.from_numpy(np.array(img)).to(gpu)                 # (a copy: the golden arrays are read-only)


def _small_chain():
    """37 x 29 down to 1 x 1: 80 + 20 + 6 + 1 + 1 + 1 = 109 blocks."""
    import itw_amd
    return itw_amd.mip_chain(np.ascontiguousarray(_etc1.ramp()[:29, :37]))


# ---- the chain ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", THRESHOLDS)
def test_full_2d_chain_equals_the_reference(itw, gpu, t):
    import torch
    levels = _small_chain()
    assert [lv.shape[:2] for lv in levels] == [(29, 37), (14, 18), (7, 9), (3, 4), (1, 2), (1, 1)]
    want = _ref_chain(levels, t, "small")
    assert want.size == 109 * 8 == itw.chain_bytes("etc1", levels)
    st = itw.EtcSettings(t)
    ok, got = itw.compress_chain("etc1", levels, settings=st)
    assert ok
    _same(got, want, "host")
    ok, got = itw.compress_chain("etc1", [_device(gpu, lv) for lv in levels], settings=st)
    torch.cuda.synchronize()
    assert ok and got.is_cuda
    _same(got, want, "device")
    ok, got = itw.compress_chain("etc1", [_device(gpu, lv) for lv in levels], settings=st, out=np.zeros(want.size, np.uint8))
    assert ok
    _same(got, want, "device images, host target")
    views, dviews = [], []
    for lv in levels:                                          # rows longer than the image, host and device (a stride that is no multiple of 16)
        h, w = lv.shape[:2]
        base = np.full((h, w + 13, 4), 7, dtype=np.uint8)
        base[:, :w] = lv
        views.append(base[:, :w])
        dbase = torch.zeros((h, w + 3, 4), dtype=torch.uint8, device=gpu)
        dbase[:, :w] = torch.from_numpy(lv).to(gpu)
        dviews.append(dbase[:, :w])
    ok, got = itw.compress_chain("etc1", views, settings=st)
    assert ok
    _same(got, want, "host, strided rows")
    ok, got = itw.compress_chain("etc1", dviews, settings=st)
    torch.cuda.synchronize()
    assert ok
    _same(got, want, "device, strided rows")
    buf = np.empty(sum(lv.nbytes for lv in levels) + 1, dtype=np.uint8)      # every image at an odd host address
    odd, off = [], 1 if buf.ctypes.data % 2 == 0 else 0
    for lv in levels:
        v = buf[off:off + lv.nbytes].reshape(lv.shape)
        v[...] = lv
        assert v.ctypes.data % 2 == 1 or lv.nbytes % 2 == 0
        odd.append(v)
        off += lv.nbytes
    assert odd[0].ctypes.data % 2 == 1
    ok, got = itw.compress_chain("etc1", odd, settings=st)
    assert ok
    _same(got, want, "host, odd addresses")


def test_default_settings_are_the_slow_preset_and_a_callers_function_gets_the_literal_loop(itw, gpu):
    levels = _small_chain()
    want = _ref_chain(levels, 6, "small")
    ok, got = itw.compress_chain("etc1", levels)
    assert ok
    _same(got, want, "default = etc_profile('slow')")
    ok, got = itw.compress_chain("etc1", levels, profile="slow")
    assert ok
    _same(got, want, "profile='slow'")
    seen = []
    st = itw.EtcSettings(32)

    def mine(surf, out):
        s = surf.contents
        seen.append((s.width, s.height))
        itw.lib().itwCompressBlocksETC1(surf, out, C.byref(st))

    fn = itw.abi.COMPRESSION_FUNC(mine)
    calls = []
    ok, got = itw.compress_chain("etc1", levels, cmp_func=C.cast(fn, C.c_void_p), progress=lambda i, n, u: calls.append((i, n)) or True)
    assert ok and calls == [(i, len(levels)) for i in range(1, len(levels) + 1)]
    assert seen == [((lv.shape[1] + 3) & ~3, (lv.shape[0] + 3) & ~3) for lv in levels]          # padded as for BC1, once per image, in order
    _same(got, _ref_chain(levels, 32, "small"), "literal loop")


@pytest.mark.parametrize("t", THRESHOLDS)
def test_cube_with_mips_in_ktx_order_and_in_dds_order(itw, gpu, golden, t):
    import torch
    names = ["noise", "ramp", "ramp", "noise", "noise", "ramp"]
    faces = [itw.mip_chain(np.ascontiguousarray(golden[n])) for n in names]         # level 0 of every face is a golden input
    mips = len(faces[0])
    assert mips == 7
    tails = {n: _ref_chain(itw.mip_chain(np.ascontiguousarray(golden[n]))[1:], t, "tail " + n) for n in ("noise", "ramp")}
    per_face = [np.concatenate([golden[f"{n}.t{_golden_threshold(t)}"], tails[n]]) for n in names]
    st = itw.EtcSettings(t)
    dds_order = [lv for face in faces for lv in face]
    want_dds = np.concatenate(per_face)
    ok, got = itw.compress_chain("etc1", dds_order, settings=st)
    assert ok
    _same(got, want_dds, "DDS order, host")
    ktx_order = [faces[f][m] for m in range(mips) for f in range(6)]
    ends = np.cumsum([0] + [((lv.shape[0] + 3) // 4) * ((lv.shape[1] + 3) // 4) * 8 for lv in faces[0]])
    want_ktx = np.concatenate([per_face[f][ends[m]:ends[m + 1]] for m in range(mips) for f in range(6)])
    ok, got = itw.compress_chain("etc1", [_device(gpu, lv) for lv in ktx_order], settings=st)
    torch.cuda.synchronize()
    assert ok
    _same(got, want_ktx, "KTX order, device")
    # ... which is a KTX file's payload, image by image
    pieces = np.split(_host(got), np.cumsum([((lv.shape[0] + 3) // 4) * ((lv.shape[1] + 3) // 4) * 8 for lv in ktx_order])[:-1])
    data = itw.ktx_file(64, 64, pieces, mip_levels=mips, cubemap=True)
    desc = itw.KtxDesc()
    assert itw.lib().itwKtxReadHeader(data.ctypes.data, data.size, C.byref(desc)) == 64 and desc.is_cubemap == 1 and desc.mip_levels == mips
    for (h, w, off, n), lv, piece in zip(itw.ktx_images(desc), ktx_order, pieces):
        assert (h, w) == lv.shape[:2] and np.array_equal(data[off:off + n], piece)


@pytest.mark.parametrize("t", THRESHOLDS)
def test_images_at_offsets_that_are_odd_multiples_of_8(itw, gpu, golden, t):
    import torch
    ramp = golden["ramp"]
    sizes = [(4, 4), (4, 12), (20, 4), (9, 9), (3, 5), (64, 64), (1, 1), (12, 12)]                # 1, 3, 5, 9, 2, 256, 1, 9 blocks
    levels = [np.ascontiguousarray(ramp[:h, :w]) for h, w in sizes]
    starts = np.cumsum([0] + [((h + 3) // 4) * ((w + 3) // 4) for h, w in sizes])[:-1]
    assert [int(s) % 2 for s in starts] == [0, 1, 0, 1, 0, 0, 0, 1]                              # images 1, 3 and 7 start at odd multiples of 8 bytes
    want = _ref_chain(levels, t, "odd")
    assert np.array_equal(want[starts[5] * 8:starts[6] * 8], golden[f"ramp.t{_golden_threshold(t)}"])
    st = itw.EtcSettings(t)
    ok, got = itw.compress_chain("etc1", levels, settings=st)
    assert ok
    _same(got, want, "host")
    for device in (None, gpu):                                                                   # the target itself 8 bytes past a multiple of 16
        g = guarded(want.size, device=device, align=16, offset=8)
        assert g.ptr % 16 == 8
        src = levels if device is None else [_device(gpu, lv) for lv in levels]
        ok, _ = itw.compress_chain("etc1", src, settings=st, out=g.view)
        if device is not None:
            torch.cuda.synchronize()
        assert ok
        g.check(f"chain into a target at 8 mod 16 ({'host' if device is None else 'device'})")
        _same(g.host(), want, "target at 8 mod 16")


@pytest.mark.parametrize("t", THRESHOLDS)
def test_a_second_packed_row_with_one_block_in_it(itw, gpu, golden, t):
    """128 x 128 plus 1 x 1: 1 025 blocks, one more than a packed row holds -- the second row's 1 023 other slots are encoded and dropped."""
    import torch
    big = _tiled(golden, "noise", 2, 2)
    one = np.ascontiguousarray(golden["ramp"][5:6, 7:8])
    want = np.concatenate([_tiled_stream(golden, "noise", t, 2, 2), _ref_chain([one], t, "one texel")])
    assert want.size == 1025 * 8
    st = itw.EtcSettings(t)
    for device in (None, gpu):
        g = guarded(want.size, device=device)
        src = [big, one] if device is None else [_device(gpu, big), _device(gpu, one)]
        ok, _ = itw.compress_chain("etc1", src, settings=st, out=g.view)
        if device is not None:
            torch.cuda.synchronize()
        assert ok
        g.check("1 025 blocks")
        _same(g.host(), want, ("1 025 blocks", device))


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("t", (6, 32))
def test_the_group_budget_of_131072_blocks_and_one_block_more(itw, gpu, golden, t, extra):
    """Four 1024 x 512 images are 4 x 32 768 = 131 072 blocks: exactly one group.  A 1 x 1 image behind them is block 131 073: a second group."""
    names = ["noise", "ramp", "ramp", "noise"]
    levels = [_tiled(golden, n, 8, 16) for n in names]
    parts = [_tiled_stream(golden, n, t, 8, 16) for n in names]
    if extra:
        one = np.ascontiguousarray(golden["noise"][9:10, 3:4])
        levels.append(one)
        parts.append(_ref_chain([one], t, "one texel b"))
    want = np.concatenate(parts)
    assert want.size == (131072 + extra) * 8
    calls = []
    g = guarded(want.size)
    ok, _ = itw.compress_chain("etc1", levels, settings=itw.EtcSettings(t), out=g.view, progress=lambda i, n, u: calls.append(i) or True)
    assert ok and calls == list(range(1, len(levels) + 1))
    g.check("budget boundary")
    _same(g.host(), want, ("budget", extra))


def test_several_groups_in_place_images_and_an_unaligned_group_of_its_own(itw, gpu, golden):
    """Threshold 1.  One 2048 x 1024 aligned image (131 072 blocks: encoded in place), twenty 512^2 images (8 + 8 + 4: three groups), one
    2046 x 1022 image (131 072 blocks after padding: a gathered group of its own)."""
    import torch
    t = 1
    st = itw.EtcSettings(t)
    levels = [_tiled(golden, "ramp", 16, 32)]
    parts = [_tiled_stream(golden, "ramp", t, 16, 32)]
    for i in range(20):
        n = ("noise", "ramp")[i % 2]
        levels.append(_tiled(golden, n, 8, 8))
        parts.append(_tiled_stream(golden, n, t, 8, 8))
    unaligned = np.ascontiguousarray(_tiled(golden, "noise", 16, 32)[:1022, :2046])
    levels.append(unaligned)
    last = _loop(itw, [unaligned], st)                      # its last block row and column hold replicated texels: this library's own pad + block call
    inner = _tiled_stream(golden, "noise", t, 16, 32).reshape(256, 512, 8)
    assert np.array_equal(last.reshape(256, 512, 8)[:255, :511], inner[:255, :511])
    parts.append(last)
    want = np.concatenate(parts)
    assert want.size == (131072 + 20 * 16384 + 131072) * 8
    ok, got = itw.compress_chain("etc1", levels, settings=st)
    assert ok
    _same(got, want, "host")
    ok, got = itw.compress_chain("etc1", [_device(gpu, lv) for lv in levels], settings=st)
    torch.cuda.synchronize()
    assert ok
    _same(got, want, "device")


@pytest.mark.parametrize("where", ["host", "device"])
def test_chain_progress_in_order_and_abort(itw, gpu, golden, where):
    names = ["noise", "ramp", "ramp", "noise", "noise", "ramp"]
    levels = [lv for n in names for lv in itw.mip_chain(np.ascontiguousarray(golden[n]))[:3]]    # 18 images: 64, 32, 16 squared
    t = 32
    per = {n: np.concatenate([golden[f"{n}.t32"], _ref_chain(itw.mip_chain(np.ascontiguousarray(golden[n]))[1:3], t, "two " + n)]) for n in ("noise", "ramp")}
    want = np.concatenate([per[n] for n in names])
    ends = np.cumsum([(lv.shape[0] // 4) * (lv.shape[1] // 4) * 8 for lv in levels])
    n = len(levels)
    src = levels if where == "host" else [_device(gpu, lv) for lv in levels]
    st = itw.EtcSettings(t)
    calls = []
    ok, got = itw.compress_chain("etc1", src, settings=st, progress=lambda i, c, u: calls.append((i, c)) or True)
    assert ok and calls == [(i, n) for i in range(1, n + 1)]
    _same(got, want, "with progress")
    for k in (1, n // 2, n):
        calls = []
        ok, got = itw.compress_chain("etc1", src, settings=st, progress=lambda i, c, u: calls.append(i) or i != k)
        assert ok is False and calls == list(range(1, k + 1)), (k, calls)
        assert itw.lib().itwLastError() is None                 # an early out is not a failure
        written = int(ends[k - 1])                               # images < k are in `target`
        assert first_mismatch(_host(got)[:written], want[:written], 8) is None, k


def test_mixed_host_and_device_images_are_refused(itw, gpu, golden):
    a = np.ascontiguousarray(golden["ramp"])
    b = _device(gpu, golden["noise"])
    out = np.full(8192, 0xA5, np.uint8)
    itw.set_error_mode(itw.ON_ERROR_RETURN)
    try:
        itw.lib().itwClearError()
        ok, _ = itw.compress_chain("etc1", [a, b], out=out)
        assert ok is False and "host" in (itw.last_error() or "")
        fn = itw.abi.COMPRESSION_FUNC(lambda s, o: None)
        itw.lib().itwClearError()
        ok, _ = itw.compress_chain("etc1", [a, b], out=out, cmp_func=C.cast(fn, C.c_void_p))
        assert ok is False and itw.last_error()
        assert (out == 0xA5).all()
    finally:
        itw.set_error_mode(itw.ON_ERROR_ABORT)
        itw.lib().itwClearError()


# ---- slices -------------------------------------------------------------------------------------------------------------------------------------
SLICED = {"256 in 16": (4, 4, 4096, 16), "1024 in 64": (16, 16, 0x4000, 64)}


@pytest.mark.parametrize("window", [1, 5, 0])               # the reference's granularity, windows that do not divide the slices, the default rule
@pytest.mark.parametrize("case", list(SLICED))
@pytest.mark.parametrize("t", THRESHOLDS)
def test_sliced_pipeline(itw, gpu, golden, slice_window, t, case, window):
    import torch
    ty, tx, slice_pixels, slices = SLICED[case]
    name = "ramp" if case == "256 in 16" else "noise"
    img = _tiled(golden, name, ty, tx)
    want = _tiled_stream(golden, name, t, ty, tx)
    st = itw.EtcSettings(t)
    slice_window(window)
    for src in (img, _device(gpu, img)):
        calls = []
        ok, out = itw.compress_image("etc1", src, slice_pixels=slice_pixels, settings=st, progress=lambda i, n, u: calls.append((i, n)) or True)
        if hasattr(out, "cpu"):
            torch.cuda.synchronize()
        assert ok and calls == [(i, slices) for i in range(1, slices)], calls[:4]
        _same(out, want, (case, window, hasattr(src, "data_ptr")))


def test_sliced_default_settings_width_4_and_a_partial_block_row(itw, gpu, golden, slice_window):
    ok, out = itw.compress_image("etc1", _tiled(golden, "ramp", 4, 4), slice_pixels=4096)
    assert ok
    _same(out, _tiled_stream(golden, "ramp", 6, 4, 4), "default = etc_profile('slow')")
    column = np.ascontiguousarray(np.tile(golden["ramp"][:, :4], (4, 1, 1)))                  # 4 wide, 256 high: 64 blocks in 16 slices
    want = np.tile(golden["ramp.t32"].reshape(16, 16, 8)[:, 0], (4, 1)).reshape(-1)
    for window in (1, 0):
        slice_window(window)
        for src in (column, _device(gpu, column)):
            calls = []
            ok, out = itw.compress_image("etc1", src, slice_pixels=64, settings=itw.EtcSettings(32), progress=lambda i, n, u: calls.append(i) or True)
            assert ok and calls == list(range(1, 16))
            _same(out, want, ("width 4", window))
    slice_window(0)
    odd = np.ascontiguousarray(_tiled(golden, "noise", 2, 2)[:127, :126])                    # partial blocks are dropped: 31 x 31 blocks
    ok, out = itw.compress_image("etc1", odd, slice_pixels=1000, settings=itw.EtcSettings(1))
    assert ok and out.size == 31 * 31 * 8
    _same(out, _tiled_stream(golden, "noise", 1, 2, 2).reshape(32, 32, 8)[:31, :31].reshape(-1), "partial blocks dropped")


@pytest.mark.parametrize("where", ["host", "device"])
def test_a_callers_function_runs_the_slices_as_the_literal_loop(itw, gpu, golden, where):
    img = _tiled(golden, "noise", 4, 4)
    want = _tiled_stream(golden, "noise", 32, 4, 4)
    st = itw.EtcSettings(32)
    seen = []

    def mine(surf, out):
        seen.append(surf.contents.height)
        itw.lib().itwCompressBlocksETC1(surf, out, C.byref(st))

    fn = itw.abi.COMPRESSION_FUNC(mine)
    src = img if where == "host" else _device(gpu, img)
    out = np.zeros(want.size, np.uint8) if where == "host" else _device(gpu, np.zeros(want.size, np.uint8))
    ptr = (lambda x: x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data)
    surf = itw.RgbaSurface(ptr(src), 256, 256, 1024)
    calls = []
    cb = itw.PROGRESS_FUNC(lambda i, n, u: calls.append(i) or True)
    ok = itw.lib().itwCompressImageSliced(C.byref(surf), ptr(out), 64 * 8, C.cast(fn, C.c_void_p), _etc1.ETC1, False, 4096, C.cast(cb, C.c_void_p), None)
    assert ok and seen == [16] * 16 and calls == list(range(1, 16))
    _same(out, want, "literal loop")


@pytest.mark.parametrize("k", [1, 32, 63])
def test_sliced_abort_leaves_the_earlier_slices_written(itw, gpu, golden, slice_window, k):
    import torch
    img = _tiled(golden, "ramp", 16, 16)
    want = _tiled_stream(golden, "ramp", 1, 16, 16)
    slice_bytes = 4 * 256 * 8                                  # 64 slices of 16 texel rows
    st = itw.EtcSettings(1)
    for window in (1, 0):
        slice_window(window)
        for src in (img, _device(gpu, img)):
            calls = []
            ok, out = itw.compress_image("etc1", src, slice_pixels=0x4000, settings=st, progress=lambda i, n, u: calls.append(i) or i != k)
            if hasattr(out, "cpu"):
                torch.cuda.synchronize()
            assert ok is False and calls == list(range(1, k + 1)), (window, calls[-3:])
            assert itw.lib().itwLastError() is None
            done = k * slice_bytes
            assert first_mismatch(_host(out)[:done], want[:done], 8) is None, (window, k)
    slice_window(0)
    ok, out = itw.compress_image("etc1", img, slice_pixels=0x4000, settings=st, progress=lambda i, n, u: True)      # the next call starts clean
    assert ok
    _same(out, want, "after the aborts")


@pytest.mark.parametrize("where", ["host", "device"])
def test_a_sliced_call_writes_its_blocks_and_nothing_else(itw, gpu, golden, slice_window, where):
    """8 bytes per block: a 16-byte stride would run 64 KiB past the end of this target."""
    import torch
    img = _tiled(golden, "noise", 4, 4)
    want = _tiled_stream(golden, "noise", 6, 4, 4)
    device = None if where == "host" else gpu
    for window in (1, 0):
        slice_window(window)
        for with_progress in (False, True):
            g = guarded(want.size, device=device, lead=2 * want.size)
            src = img if device is None else _device(gpu, img)
            ok, _ = itw.compress_image("etc1", src, slice_pixels=4096, settings=itw.EtcSettings(6), out=g.view,
                                       progress=(lambda i, n, u: True) if with_progress else None)
            if device is not None:
                torch.cuda.synchronize()
            assert ok
            g.check(f"sliced, window {window}, progress {with_progress}, {where}")
            _same(g.host(), want, "sliced into a guarded target")


@pytest.mark.parametrize("where", ["host", "device"])
def test_a_chain_call_writes_its_blocks_and_nothing_else(itw, gpu, golden, where):
    import torch
    levels = _small_chain() + [np.ascontiguousarray(golden["noise"])] + _small_chain()
    want = np.concatenate([_ref_chain(_small_chain(), 6, "small"), golden["noise.t6"], _ref_chain(_small_chain(), 6, "small")])
    device = None if where == "host" else gpu
    g = guarded(want.size, device=device, lead=2 * want.size + 65536)
    src = levels if device is None else [_device(gpu, lv) for lv in levels]
    ok, _ = itw.compress_chain("etc1", src, out=g.view)
    if device is not None:
        torch.cuda.synchronize()
    assert ok
    g.check("chain, " + where)
    _same(g.host(), want, "chain into a guarded target")


# ---- the file -----------------------------------------------------------------------------------------------------------------------------------
def _numpy_sums(stream, levels):
    """Per image: (decoded texels, [sum of squared differences of R, G, B]) by the numpy decoder, over the texels inside the image."""
    out, off = [], 0
    for lv in levels:
        h, w = lv.shape[:2]
        ph, pw = (h + 3) & ~3, (w + 3) & ~3
        n = (ph // 4) * (pw // 4) * 8
        texels, _ = _etc1.decode_np(stream[off:off + n], pw, ph)
        texels = texels[:h, :w]
        d = texels[..., :3].astype(np.int64) - lv[..., :3].astype(np.int64)
        out.append((texels, [int((d[..., c] ** 2).sum()) for c in range(3)]))
        off += n
    return out


@pytest.mark.parametrize("device", [False, True])
def test_round_trip_through_a_ktx_file(itw, gpu, device):
    import torch
    levels = _small_chain()
    want = _ref_chain(levels, 6, "small")
    ok, stream = itw.compress_chain("etc1", levels)
    assert ok
    pieces = np.split(stream, np.cumsum([((lv.shape[0] + 3) // 4) * ((lv.shape[1] + 3) // 4) * 8 for lv in levels])[:-1])
    data = itw.ktx_file(37, 29, pieces, mip_levels=len(levels))                      # (a 2D texture: KTX order is the mip order)
    desc, texels, amin = itw.load_ktx(data.tobytes(), device=gpu if device else None)
    assert (desc.width, desc.height, desc.mip_levels, desc.is_cubemap) == (37, 29, 6, 0) and amin == [255] * 6
    expect = _numpy_sums(want, levels)
    for got, (tex, _), lv in zip(texels, expect, levels):
        got = _host(got)
        assert got.shape == lv.shape and np.array_equal(got, tex)
    loaded = np.concatenate([data[off:off + n] for _, _, off, n in itw.ktx_images(desc)])
    assert np.array_equal(loaded, want)
    stats = itw.measure_chain("etc1", _device(gpu, loaded) if device else loaded, [_device(gpu, lv) for lv in levels] if device else levels)
    for s, (_, sse), lv in zip(stats, expect, levels):
        assert [int(v) for v in s.sse[:3]] == sse and (s.width, s.height) == (lv.shape[1], lv.shape[0])


def test_encode_dds_writes_measures_and_decodes_a_ktx_file(itw, gpu, golden, tmp_path):
    exe = os.path.join(ROOT, "examples", "encode_dds")
    assert os.path.exists(exe), "examples/encode_dds is missing: build() makes it"
    img = golden["ramp"]
    raw, ktx, back = tmp_path / "in.raw", tmp_path / "out.ktx", tmp_path / "back.raw"
    raw.write_bytes(img.tobytes())
    r = subprocess.run([exe, "--measure", "etc1_slow", "64", "64", str(raw), str(ktx), "1024"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want = golden["ramp.t6"]
    assert ktx.read_bytes() == itw.ktx_file(64, 64, [want]).tobytes()
    (_, sse), = _numpy_sums(want, [img])
    assert f"sse [{sse[0]}, {sse[1]}, {sse[2]}, 0]" in r.stdout and "etc1_slow" in r.stdout, r.stdout
    assert "slice 3 / 4" in r.stderr                            # 4 096 pixels in slices of 1 024
    r = subprocess.run([exe, "--decode", str(ktx), str(back)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "image 0: 64 64 min_alpha 255"
    assert back.read_bytes() == _etc1.decode_np(want, 64, 64)[0].tobytes()
    r = subprocess.run([exe, "--refine", "slow", "100", "etc1_slow", "64", "64", str(raw), str(ktx)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "ETC1" in r.stderr
