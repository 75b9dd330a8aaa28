"""ETC1 on the GPU: itwCompressBlocksETC1 is the reference's CompressBlocksETC1 byte for byte (live library and golden file), whatever the
pointers, the stride, the alpha and the size; the device decoder and the measuring kernel agree with the numpy decoder of tests/_etc1.py on
every table pair, flip, base encoding and delta; every entry point writes its output and nothing else; a device-pointer call can be captured."""
import ctypes as C

import numpy as np
import pytest

import _etc1
from _guarded import frozen, guarded, rows_of
from conftest import first_mismatch

pytestmark = pytest.mark.gpu

THRESHOLDS = (1, 2, 6, 32, 165)
INPUTS = {"noise": _etc1.noise, "ramp": _etc1.ramp}


@pytest.fixture(scope="module")
def golden():
    return _etc1.load_golden()


def _same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    m = first_mismatch(got, want, 8)
    assert got.size == want.size and m is None, (what, m)


def _device(gpu, img):
    import torch
    return torch.from_numpy(np.ascontiguousarray(img)).to(gpu)


# ---- parity -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def covered():
    """The reference streams the parity tests compare against take every path: a pass cannot come from inputs that skip one."""
    _etc1.live_reference()
    both = _etc1.coverage([_etc1.ref_stream("noise", 6), _etc1.ref_stream("ramp", 6)])
    assert both["pairs"] == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert both["table0"] == set(range(8)) and both["table1"] == set(range(8))
    r = _etc1.coverage([_etc1.ref_stream("ramp", 6)])
    # the inputs are seeded and the reference is pinned, so the counts are exact: 72 of ramp's 168 differential blocks have a delta at -4 or +3
    # (the issue counted 63 of 168 on its own draw of the same construction)
    assert (r["differential"], r["clamped"]) == (168, 72), r


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("name", ["noise", "ramp"])
def test_parity_with_the_live_reference(itw, gpu, covered, name, threshold):
    import torch
    img = INPUTS[name]()
    want = _etc1.ref_stream(name, threshold)
    st = itw.EtcSettings(threshold)
    _same(itw.compress("etc1", _device(gpu, img), st), want, (name, threshold, "device"))
    torch.cuda.synchronize()
    _same(itw.compress_numpy("etc1", img, st), want, (name, threshold, "host"))


@pytest.mark.parametrize("name", ["noise", "ramp"])
def test_threshold_above_165_is_165(itw, gpu, covered, name):
    _same(itw.compress("etc1", _device(gpu, INPUTS[name]()), itw.EtcSettings(200)), _etc1.ref_stream(name, 165), name)
    _same(itw.compress_numpy("etc1", INPUTS[name](), itw.EtcSettings(200)), _etc1.ref_stream(name, 165), name)


@pytest.mark.parametrize("threshold", _etc1.GOLDEN_THRESHOLDS)
@pytest.mark.parametrize("name", ["noise", "ramp"])
def test_parity_with_the_golden_file(itw, gpu, golden, name, threshold):
    st = itw.EtcSettings(threshold)
    _same(itw.compress("etc1", _device(gpu, golden[name]), st), golden[f"{name}.t{threshold}"], (name, threshold, "device"))
    _same(itw.compress_numpy("etc1", golden[name], st), golden[f"{name}.t{threshold}"], (name, threshold, "host"))


def test_default_settings_are_the_slow_profile(itw, gpu, golden):
    _same(itw.compress("etc1", _device(gpu, golden["ramp"])), golden["ramp.t6"], "default")
    _same(itw.compress("etc1", _device(gpu, golden["ramp"]), "slow"), golden["ramp.t6"], "slow")


@pytest.mark.parametrize("name", ["noise", "ramp"])
def test_strided_rows(itw, gpu, golden, name):
    """64 texels wide inside rows of 80"""
    wide = np.full((64, 80, 4), 0xC3, dtype=np.uint8)
    wide[:, :64] = golden[name]
    want = golden[f"{name}.t6"]
    _same(itw.compress("etc1", _device(gpu, wide)[:, :64], itw.EtcSettings(6)), want, (name, "device"))
    _same(itw.compress_numpy("etc1", wide[:, :64], itw.EtcSettings(6)), want, (name, "host"))


def test_source_alpha_is_ignored(itw, gpu, golden):
    img = golden["ramp"].copy()
    img[..., 3] = np.random.default_rng(9).integers(0, 256, (64, 64), dtype=np.uint8)
    _same(itw.compress("etc1", _device(gpu, img), itw.EtcSettings(6)), golden["ramp.t6"], "device")
    _same(itw.compress_numpy("etc1", img, itw.EtcSettings(6)), golden["ramp.t6"], "host")


# ---- geometry -----------------------------------------------------------------------------------------------------------------------------------
# one block; three blocks: less than a wave's worth of workgroup; 65 x 2 blocks; five blocks: one past a workgroup (a workgroup encodes four
# blocks, one per wave; the kernel has no grid stride); sizes that are no multiple of 4 drop the partial blocks like BC1
@pytest.mark.parametrize("w,h", [(4, 4), (12, 4), (260, 8), (20, 4), (23, 9)], ids=lambda v: str(v))
def test_geometry(itw, gpu, w, h):
    _etc1.live_reference()
    img = np.ascontiguousarray(np.tile(_etc1.ramp(), (1, 5, 1))[:h, :w])
    want = _etc1.ref_encode(np.ascontiguousarray(img[:h // 4 * 4, :w // 4 * 4]), 6)
    assert want.size == (w // 4) * (h // 4) * 8
    _same(itw.compress("etc1", _device(gpu, img), itw.EtcSettings(6)), want, (w, h, "device"))
    _same(itw.compress_numpy("etc1", img, itw.EtcSettings(6)), want, (w, h, "host"))


# ---- the decoder ----------------------------------------------------------------------------------------------------------------------------------
SWEEP_W, SWEEP_H = 252, 256                                      # 63 x 64 = 4 032 blocks


def _sweep():
    """Every table pair x flip x diff with random bases and index planes (12 of each), and every delta -4 .. 3 against the bases 0, 1, 15,
    30 and 31 in each channel, so that valid and overflowing sums both occur."""
    rng = np.random.default_rng(77)
    blocks = []
    for t0 in range(8):
        for t1 in range(8):
            for flip in (0, 1):
                for diff in (0, 1):
                    for _ in range(12):
                        b = rng.integers(0, 256, 8, dtype=np.uint8)
                        b[3] = (t0 << 5) | (t1 << 2) | (diff << 1) | flip
                        blocks.append(b)
    for delta in range(-4, 4):
        for base in (0, 1, 15, 30, 31):
            for channel in range(3):
                for _ in range(8):
                    b = rng.integers(0, 256, 8, dtype=np.uint8)
                    b[3] = (b[3] & 0xFD) | 2
                    for c in range(3):                           # the other channels: a sum that stays in range
                        b[c] = (int(rng.integers(4, 28)) << 3) | int(rng.integers(0, 8))
                    b[channel] = (base << 3) | (delta & 7)
                    blocks.append(b)
    out = np.concatenate(blocks)
    assert out.size == (SWEEP_W // 4) * (SWEEP_H // 4) * 8
    return out


@pytest.fixture(scope="module")
def sweep():
    blocks = _sweep()
    texels, modes = _etc1.decode_np(blocks, SWEEP_W, SWEEP_H)
    assert set(modes.tolist()) == {-1, 0, 1} and (modes == -1).sum() >= 100
    for a in (blocks, texels, modes):
        a.setflags(write=False)
    return blocks, texels, modes


@pytest.mark.parametrize("where", ["host", "device"])
def test_decode_blocks_sweep(itw, gpu, sweep, where):
    import torch
    blocks, want, want_modes = sweep
    src = blocks if where == "host" else torch.from_numpy(blocks.copy()).to(gpu)
    got, modes = itw.decode("etc1", src, SWEEP_W, SWEEP_H, want_modes=True)
    if where == "device":
        got, modes = got.cpu().numpy(), modes.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    assert np.array_equal(modes, want_modes)


@pytest.mark.parametrize("where", ["host", "device"])
def test_decode_image_sweep(itw, gpu, sweep, where):
    import torch
    blocks, want, want_modes = sweep
    src = blocks if where == "host" else torch.from_numpy(blocks.copy()).to(gpu)
    got, modes, amin = itw.decode_image("etc1", src, (SWEEP_H, SWEEP_W), want_modes=True, want_min_alpha=True)
    if where == "device":
        got, modes, amin = got.cpu().numpy(), modes.cpu().numpy(), int(amin.cpu()[0])
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    assert np.array_equal(modes, want_modes) and amin == 255


def test_decode_image_into_a_30x30_view_of_a_larger_canvas(itw, gpu, sweep):
    import torch
    blocks = sweep[0][2048 * 8:(2048 + 64) * 8]                  # 8 x 8 blocks, raster order of a 32 x 32 image
    want, want_modes = _etc1.decode_np(blocks, 32, 32)
    canvas = torch.full((40, 48, 4), 0x5A, dtype=torch.uint8, device=gpu)
    view = canvas[3:33, 5:35]
    got, modes = itw.decode_image("etc1", torch.from_numpy(blocks.copy()).to(gpu), view, want_modes=True)
    torch.cuda.synchronize()
    host = canvas.cpu().numpy()
    assert np.array_equal(host[3:33, 5:35], want[:30, :30])
    host[3:33, 5:35] = 0x5A
    assert (host == 0x5A).all()                                  # the cropped edge blocks wrote nothing outside the view
    assert np.array_equal(modes.cpu().numpy(), want_modes)


def test_decode_blocks_refuses_partial_blocks_and_the_encode_side_refuses_the_format(itw, gpu, sweep):
    out = np.zeros((32, 32, 4), dtype=np.uint8)
    assert itw.lib().itwDecodeBlocks(_etc1.ETC1, sweep[0].ctypes.data, 30, 30, out.ctypes.data, 128, None) == -1
    assert itw.lib().GetBytesPerBlock(_etc1.ETC1) == 8           # "anything unknown": the dispatch layer does not know the code
    assert itw.psnr_to_total_sse("etc1", 64, 64, 40.0) == 2 ** 64 - 1                      # refining does not know it either


# ---- measuring --------------------------------------------------------------------------------------------------------------------------------
def _expected_stats(blocks, src):
    h, w = src.shape[:2]
    texels, modes = _etc1.decode_np(blocks, w, h)
    d = texels.astype(np.int64) - src.astype(np.int64)
    per_block = (d * d).reshape(h // 4, 4, w // 4, 4, 4).sum(axis=(1, 3, 4)).reshape(-1)
    return {"dxgi_format": _etc1.ETC1, "width": w, "height": h, "blocks": modes.size, "reserved_blocks": int((modes == -1).sum()),
            "sse": [int((d[..., c] ** 2).sum()) for c in range(4)], "max_abs": [int(np.abs(d[..., c]).max()) for c in range(4)],
            "worst_block_sse": int(per_block.max()), "worst_block": int(per_block.argmax()),
            "mode_hist": [int((modes == 0).sum()), int((modes == 1).sum())] + [0] * 14}, per_block


@pytest.mark.parametrize("case", ["encoded ramp", "sweep"])
@pytest.mark.parametrize("where", ["host", "device"])
def test_measure(itw, gpu, golden, sweep, case, where):
    import torch
    if case == "encoded ramp":
        src = golden["ramp"].copy()
        src[..., 3] = np.random.default_rng(5).integers(0, 256, (64, 64), dtype=np.uint8)      # sse[3] against the filled 255
        blocks = golden["ramp.t6"]
    else:
        src = np.random.default_rng(6).integers(0, 256, (SWEEP_H, SWEEP_W, 4), dtype=np.uint8)
        blocks = sweep[0]
    want, want_map = _expected_stats(blocks, src)
    if where == "host":
        st, bmap = itw.measure("etc1", blocks, src, want_block_map=True)
    else:
        st, bmap = itw.measure("etc1", torch.from_numpy(blocks.copy()).to(gpu), _device(gpu, src), want_block_map=True)
        bmap = bmap.cpu().numpy()
    assert st.as_dict() == want
    assert np.array_equal(np.asarray(bmap).astype(np.int64), want_map)
    assert (want["reserved_blocks"] > 0) == (case == "sweep")
    rgb = sum(want["sse"][:3])
    assert abs(st.psnr("rgb") - 10.0 * np.log10(255.0 ** 2 * src.shape[0] * src.shape[1] * 3 / rgb)) < 1e-9
    assert abs(st.psnr() - st.psnr("rgb")) == 0.0                # the format's own channels


def test_measure_blocks_and_chain_through_the_c_abi(itw, gpu, golden):
    src = golden["ramp"]
    want, _ = _expected_stats(golden["ramp.t6"], src)
    surf = itw.RgbaSurface(src.ctypes.data, 64, 64, 256)
    st = itw.ErrorStats()
    assert itw.lib().itwMeasureBlocks(_etc1.ETC1, golden["ramp.t6"].ctypes.data, C.byref(surf), C.addressof(st), C.sizeof(st), None) == 0
    assert st.as_dict() == want
    st2 = itw.ErrorStats()
    assert itw.lib().itwMeasureChain(C.byref(surf), 1, golden["ramp.t6"].ctypes.data, _etc1.ETC1, C.addressof(st2), C.sizeof(st2)) == 0
    assert st2.as_dict() == want


# ---- write extents --------------------------------------------------------------------------------------------------------------------------------
def _twice(outs, srcs, call, compare, what):
    import torch
    for rnd in (1, 2):
        for o in outs:
            o.refill()
        call()
        torch.cuda.synchronize()
        compare((what, f"call {rnd}"))
        for k, o in enumerate(outs):
            o.check(f"{what}, call {rnd}, output {k}")
        for k, s in enumerate(srcs):
            s.check(f"{what}, call {rnd}, source {k}")


@pytest.mark.parametrize("w,h", [(12, 4), (64, 64)], ids=["12x4", "64x64"])
@pytest.mark.parametrize("where", ["host", "device"])
def test_extents_of_the_encoder(itw, gpu, golden, where, w, h):
    import torch
    img = np.ascontiguousarray(golden["ramp"][:h, :w])
    if (w, h) == (64, 64):
        want = golden["ramp.t6"]
    else:
        _etc1.live_reference()
        want = _etc1.ref_encode(img, 6)
    device = gpu if where == "device" else None
    src = frozen(img, row_pad=48, device=device)
    out = guarded(want.size, device=device, align=16, offset=8)       # 8-byte aligned and no more
    st = itw.EtcSettings(6)
    itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)

    def call():
        surf = itw.RgbaSurface(src.ptr, w, h, src.stride)
        itw.lib().itwCompressBlocksETC1(C.byref(surf), out.ptr, C.byref(st))

    _twice([out], [src], call, lambda at: _same(out.host(), want, at), f"etc1 {w}x{h} {where}")
    assert itw.last_error() is None


def test_extents_of_decode_and_measure(itw, gpu, golden):
    import torch
    blocks, img = golden["ramp.t6"], golden["ramp"]
    want, want_modes = _etc1.decode_np(blocks, 64, 64)
    stats_want, map_want = _expected_stats(blocks, img)
    d_blocks = frozen(blocks, device=gpu)
    d_src = frozen(img, row_pad=48, device=gpu)
    stride = 64 * 4 + 64
    out = guarded(64 * stride, device=gpu, rows=(64, 256, stride))
    modes = guarded(256 * 4, device=gpu)
    stats = guarded(C.sizeof(itw.ErrorStats), device=gpu, offset=8)
    bmap = guarded(256 * 8, device=gpu)
    itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)

    def call():
        assert itw.lib().itwDecodeBlocks(_etc1.ETC1, d_blocks.ptr, 64, 64, out.ptr, stride, modes.ptr) == 0
        itw.measure_async("etc1", d_blocks.view, d_src.view, stats.view, bmap.view.view(torch.int64))

    def compare(at):
        assert np.array_equal(rows_of(out).reshape(64, 64, 4), want), at
        assert np.array_equal(modes.host().view(np.int32), want_modes), at
        assert itw.ErrorStats.from_buffer_copy(stats.host().tobytes()).as_dict() == stats_want, at
        assert np.array_equal(bmap.host().view(np.uint64).astype(np.int64), map_want), at

    _twice([out, modes, stats, bmap], [d_blocks, d_src], call, compare, "etc1 decode + measure")


# ---- graph capture ----------------------------------------------------------------------------------------------------------------------------------
def test_a_device_pointer_call_can_be_captured(itw, gpu, golden):
    import torch
    d = _device(gpu, golden["ramp"])
    st = itw.EtcSettings(6)
    eager = itw.compress("etc1", d, st).clone()
    torch.cuda.synchronize()
    _same(eager, golden["ramp.t6"], "eager")
    out = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        itw.compress("etc1", d, st, out=out)
    torch.cuda.synchronize()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
