"""GPU, the signed reading of BC6H (ITW_FORMAT_BC6H_SIGNED, include/itw_decode.h): every entry point that takes the code gives the bits of
the reference's D3DXDecodeBC6HS as recorded in tests/golden/bc6hs_ref.npz (tests/test_bc6hs_cpu.py holds reference == recording == model ==
the decoder's text on the host, and what the recording contains).  Only the npz is read, never the reference.  Every comparison is equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _dxtex_bc6hs as H
import _preview

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "encode_dds")
KEY = "bc6h_signed"
SENTINEL = 0xA5A5
LAYOUT = {"sweep": (256, 512), "constructed": (144, 168), "random": (256, 256)}      # width, height: whole-block images of the three sets
CHAIN = [(21, 37), (10, 18), (5, 9), (2, 4), (1, 2), (1, 1)]                         # (height, width): 37 x 21 and its mips


@pytest.fixture(scope="module")
def rec():
    """name -> (blocks flat uint8, texels (n, 16, 4) uint16, modes from the construction / the model, flags)"""
    out = {}
    for name, blocks, rgb in H.recorded_sets():
        texels = np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 0x3C00, dtype=np.uint16)], axis=2)
        m = H.model(blocks)
        assert np.array_equal(m["texels"], texels)
        out[name] = (np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1), texels, m["modes"], m)
    import _block_sweep as S
    assert np.array_equal(out["sweep"][2], S.bc6h_modes())                       # (a): the modes are the construction's
    return out


def image(texels, width, height, crop=None):
    """The (height, width, 4) image of whole-block texels, cropped to (h, w)."""
    img = H.image_of(texels, width, height)
    return img if crop is None else np.ascontiguousarray(img[:crop[0], :crop[1]])


def chain_of(rec, sizes, start=0):
    """Consecutive recorded blocks (the constructed set, then the random one) cut into a chain of `sizes`: payload, [expected images], modes."""
    blocks = np.concatenate([rec["constructed"][0], rec["random"][0]]).reshape(-1, 16)
    texels = np.concatenate([rec["constructed"][1], rec["random"][1]])
    modes = np.concatenate([rec["constructed"][2], rec["random"][2]])
    want, at = [], start
    for h, w in sizes:
        bx, by = (w + 3) // 4, (h + 3) // 4
        want.append(image(texels[at:at + bx * by], bx * 4, by * 4, (h, w)))
        at += bx * by
    return np.ascontiguousarray(blocks[start:at]).reshape(-1), want, modes[start:at]


def to_np(t):
    return t.cpu().numpy().view(np.uint16) if hasattr(t, "cpu") else t


# ---- 1. the three sets through the three decode calls -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["sweep", "constructed", "random"])
def test_sets_through_every_decode_call_and_pointer_kind(itw, gpu, rec, name):
    import torch
    blocks, texels, modes, _ = rec[name]
    w, h = LAYOUT[name]
    want = image(texels, w, h)
    L = itw.lib()
    # host pointers
    got, m = itw.decode(KEY, blocks, w, h, want_modes=True)
    assert np.array_equal(got, want) and np.array_equal(m, modes)
    got, m, amin = itw.decode_image(KEY, blocks, (h, w), want_modes=True, want_min_alpha=True)
    assert np.array_equal(got, want) and np.array_equal(m, modes) and amin == 0x3C00
    (got,), m = itw.decode_chain(KEY, blocks, [(h, w)], want_modes=True)
    assert np.array_equal(got, want) and np.array_equal(m, modes)
    # device pointers
    d_blocks = torch.from_numpy(blocks.copy()).to(gpu)
    for call in (lambda: itw.decode(KEY, d_blocks, w, h, want_modes=True), lambda: itw.decode_image(KEY, d_blocks, (h, w), want_modes=True),
                 lambda: itw.decode_chain(KEY, d_blocks, [(h, w)], want_modes=True)):
        got, m = call()
        torch.cuda.synchronize()
        got = got[0] if isinstance(got, list) else got
        assert np.array_equal(to_np(got), want) and np.array_equal(m.cpu().numpy(), modes)
    # mixed: host blocks, device texels, host modes; device blocks, host texels, device modes
    d_out = torch.full((h, w, 4), -1, dtype=torch.int16, device=gpu)
    h_modes = np.full(modes.size, -7, dtype=np.int32)
    assert L.itwDecodeBlocks(H.FORMAT, blocks.ctypes.data, w, h, d_out.data_ptr(), w * 8, h_modes.ctypes.data) == 0
    assert np.array_equal(to_np(d_out), want) and np.array_equal(h_modes, modes)
    h_out = np.full((h, w, 4), SENTINEL, dtype=np.uint16)
    d_modes = torch.full((modes.size,), -7, dtype=torch.int32, device=gpu)
    surf = itw.RgbaSurface(h_out.ctypes.data, w, h, w * 8)
    word = np.zeros(1, dtype=np.uint32)
    assert L.itwDecodeImage(H.FORMAT, d_blocks.data_ptr(), C.byref(surf), d_modes.data_ptr(), word.ctypes.data) == 0
    assert np.array_equal(h_out, want) and np.array_equal(d_modes.cpu().numpy(), modes) and word[0] == 0x3C00


# ---- 2. a chain: cropped stores into strided views, nothing else written ----------------------------------------------------------------------

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_chain_into_strided_views_of_a_guarded_canvas(itw, gpu, rec, device):
    import torch
    payload, want, modes = chain_of(rec, CHAIN, start=1390)                    # (the end of the constructed set: the 16-bit mode and its -Inf)
    assert any((wimg == 0xFC00).any() for wimg in want)
    canvas = np.full((64, 64, 4), SENTINEL, dtype=np.uint16)
    places = [(3, 5), (30, 7), (45, 9), (52, 30), (57, 41), (60, 50)]
    if device:
        canvas_d = torch.from_numpy(canvas.view(np.int16)).to(gpu)
        outs = [canvas_d[y:y + h, x:x + w] for (h, w), (y, x) in zip(CHAIN, places)]
        blocks = torch.from_numpy(payload.copy()).to(gpu)
    else:
        outs = [canvas[y:y + h, x:x + w] for (h, w), (y, x) in zip(CHAIN, places)]
        blocks = payload
    _, m, amin = itw.decode_chain(KEY, blocks, outs, want_modes=True, want_min_alpha=True)
    if device:
        torch.cuda.synchronize()
        canvas, m, amin = canvas_d.cpu().numpy().view(np.uint16), m.cpu().numpy(), amin.cpu().numpy().view(np.uint32)
    expect = np.full((64, 64, 4), SENTINEL, dtype=np.uint16)
    for (h, w), (y, x), wimg in zip(CHAIN, places, want):
        expect[y:y + h, x:x + w] = wimg
    assert np.array_equal(canvas, expect)
    assert np.array_equal(m, modes) and [int(v) for v in amin] == [0x3C00] * len(CHAIN)
    assert payload.size == itw.chain_bytes("bc6h", CHAIN)                                     # the stream is sized like 95's


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_six_faces_straight_into_a_cross_canvas(itw, gpu, rec, device):
    import torch
    payload, want, _ = chain_of(rec, [(8, 8)] * 6, start=200)
    canvas = np.full((24, 32, 4), SENTINEL, dtype=np.uint16)
    expect = canvas.copy()
    for (cx, cy), wimg in zip(((2, 1), (0, 1), (1, 0), (1, 2), (1, 1), (3, 1)), want):
        expect[cy * 8:cy * 8 + 8, cx * 8:cx * 8 + 8] = wimg
    if device:
        canvas_d = torch.from_numpy(canvas.view(np.int16)).to(gpu)
        itw.decode_chain(KEY, torch.from_numpy(payload.copy()).to(gpu), itw.cube_cross_faces(canvas_d))
        torch.cuda.synchronize()
        canvas = canvas_d.cpu().numpy().view(np.uint16)
    else:
        itw.decode_chain(KEY, payload, itw.cube_cross_faces(canvas))
    assert np.array_equal(canvas, expect)


# ---- 3. rows 8 bytes off a 16-byte address: stores that are no aligned vectors -----------------------------------------------------------------

def test_rows_eight_bytes_off_a_sixteen_byte_address(itw, gpu, rec):
    import torch
    blocks, texels, modes, _ = rec["random"]
    w, h = LAYOUT["random"]
    buf = torch.full((h, 4 * w + 8), -23131, dtype=torch.int16, device=gpu)      # 0xA5A5; a row is w * 8 + 16 bytes
    out = buf[:, 4:4 + 4 * w].unflatten(1, (w, 4))
    assert out.data_ptr() % 16 == 8 and (out.stride(0) * 2) % 16 == 0
    itw.decode_image(KEY, torch.from_numpy(blocks.copy()).to(gpu), out)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint16)
    assert np.array_equal(got[:, 4:4 + 4 * w].reshape(h, w, 4), image(texels, w, h))
    assert (got[:, :4] == SENTINEL).all() and (got[:, 4 + 4 * w:] == SENTINEL).all()


# ---- 4. measure ----------------------------------------------------------------------------------------------------------------------------

def expected_stats(decoded, modes, src):
    """itw_error_stats of a stream whose padded decode is `decoded` (H, W, 4) against `src` (h, w, 4), in the signed reading's codes."""
    h, w = src.shape[:2]
    Hp, Wp = decoded.shape[:2]
    d = H.code(src) - H.code(decoded[:h, :w])
    sq = d * d
    per = np.zeros((Hp, Wp), dtype=np.int64)
    per[:h, :w] = sq.sum(axis=2)
    bmap = per.reshape(Hp // 4, 4, Wp // 4, 4).sum(axis=(1, 3)).reshape(-1)
    hist = np.bincount(modes[modes >= 0], minlength=16)
    return {"dxgi_format": H.FORMAT, "width": w, "height": h, "reserved_blocks": int((modes < 0).sum()), "blocks": int(modes.size),
            "sse": [int(v) for v in sq.sum(axis=(0, 1))], "max_abs": [int(v) for v in np.abs(d).max(axis=(0, 1))],
            "worst_block_sse": int(bmap.max()), "worst_block": int(np.argmax(bmap)), "mode_hist": [int(v) for v in hist]}, bmap


def two_signed_source(decoded, seed):
    """The decoded texels with a band of random 16-bit patterns (NaNs among them), both zeros, both infinities and a changed alpha."""
    rng = np.random.default_rng(seed)
    src = decoded.copy()
    hh, ww = src.shape[:2]
    src[: max(1, hh // 3)] = rng.integers(0, 65536, src[: max(1, hh // 3)].shape, dtype=np.uint16)
    flat = src.reshape(-1, 4)
    for i, v in enumerate((0x0000, 0x8000, 0x7C00, 0xFC00, 0xFFFF, 0x7FFF, 0x8001)):
        flat[(i * 37 + 11) % flat.shape[0], i % 3] = v
    flat[flat.shape[0] // 2, 3] = 0xBC00                                         # alpha goes through the same map: -1.0 against 1.0
    return src


def test_measure_blocks_against_numpy(itw, gpu, rec):
    import torch
    blocks, texels, modes, _ = rec["sweep"]
    w, h = LAYOUT["sweep"]
    decoded = image(texels, w, h)
    zero, zmap = expected_stats(decoded, modes, decoded)
    assert zero["sse"] == [0] * 4 and zero["max_abs"] == [0] * 4 and zero["reserved_blocks"] == 1024 and not zmap.any()
    st, got_map = itw.measure(KEY, blocks, decoded, want_block_map=True)
    assert st.as_dict() == zero and not got_map.any()
    src = two_signed_source(decoded, 5)
    want, bmap = expected_stats(decoded, modes, src)
    assert max(want["max_abs"]) > 0x8000 and want["max_abs"][3] >= 2 * 0x3C00     # differences across 0 are wider than any unsigned code
    st, got_map = itw.measure(KEY, blocks, src, want_block_map=True)
    assert st.as_dict() == want and np.array_equal(got_map, bmap.astype(np.uint64))
    st_d = itw.measure(KEY, torch.from_numpy(blocks.copy()).to(gpu), torch.from_numpy(src.view(np.int16)).to(gpu))
    assert st_d.as_dict() == want
    assert np.isnan(itw.lib().itwStatsPsnr(C.byref(st), 7))
    # the unsigned reading of the same stream and source is another measurement
    assert itw.measure("bc6h", blocks, src).as_dict()["sse"] != want["sse"]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_measure_chain_against_numpy(itw, gpu, rec, device):
    import torch
    payload, want_imgs, modes = chain_of(rec, CHAIN, start=1390)
    padded = chain_of(rec, [((h + 3) // 4 * 4, (w + 3) // 4 * 4) for h, w in CHAIN], start=1390)[1]
    sources = [two_signed_source(wimg, 40 + i) for i, wimg in enumerate(want_imgs)]
    if device:
        res = itw.measure_chain(KEY, torch.from_numpy(payload.copy()).to(gpu), [torch.from_numpy(s.view(np.int16)).to(gpu) for s in sources])
    else:
        res = itw.measure_chain(KEY, payload, sources)
    at = 0
    for st, src, dec in zip(res, sources, padded):
        nb = (dec.shape[0] // 4) * (dec.shape[1] // 4)
        assert st.as_dict() == expected_stats(dec, modes[at:at + nb], src)[0], src.shape
        at += nb


# ---- 5. preview ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("exposure", [1.0, 0.25])
@pytest.mark.parametrize("zoom", [1.5, 3.0], ids=["tile", "per_pixel"])
def test_preview_of_a_128x128_stream(itw, gpu, rec, zoom, exposure, device):
    import torch
    blocks = rec["constructed"][0].reshape(-1, 16)[488:1512]
    texels = image(rec["constructed"][1][488:1512], 128, 128)
    assert (texels == 0xFC00).any() and ((texels[..., :3] & 0x8000) != 0).any()
    stream = np.ascontiguousarray(blocks).reshape(-1)
    for channels, x, y in (("rgb", 0, 0), ("rgba", -3, 5), ("g", 2, 6)):
        view = dict(view_w=96, view_h=80, x=x, y=y, zoom=zoom, channels=channels, matte=0x00336699, exposure=exposure)
        if device:
            got = itw.preview(KEY, torch.from_numpy(stream.copy()).to(gpu), 128, 128, **view)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
        else:
            got = itw.preview(KEY, stream, 128, 128, **view)
        options = sum({"r": 4, "g": 8, "b": 16, "a": 32}[c] for c in channels)
        want = _preview.viewport(texels, 96, 80, x, y, zoom, options, 0x00336699, exposure)
        assert got.shape == want.shape and np.array_equal(got, want), (channels, zoom, np.argwhere((got != want).any(axis=2))[:4])
        if channels == "g":                                                      # a negative half, -Inf included, shows 0
            in_y, sy = _preview.coords(80, y, zoom, 128)
            in_x, sx = _preview.coords(96, x, zoom, 128)
            shown = texels[sy[:, None], sx[None, :], 1]
            neg = (in_y[:, None] & in_x[None, :]) & ((shown & 0x8000) != 0)
            assert neg.any() and (shown[neg] == 0xFC00).any() and (got[neg] == 0).all()


# ---- 6. the load path ------------------------------------------------------------------------------------------------------------------------

def test_a_bc6h_sf16_file_is_read_as_a_gpu_reads_it(itw, gpu, rec, tmp_path):
    import torch
    sizes = [(16 >> l, 16 >> l) for _ in range(6) for l in range(5)]
    payload, want, _ = chain_of(rec, sizes, start=1380)
    counts = [16 * ((h + 3) // 4) * ((w + 3) // 4) for h, w in sizes]
    levels = np.split(payload, np.cumsum(counts)[:-1])
    f = itw.dds_file("bc6h_sf16", 16, 16, levels, mip_levels=5, cubemap=True)
    assert f.size == 148 + payload.size and f[84:88].tobytes() == b"DX10" and int(f[128:132].view(np.uint32)[0]) == 96
    for device in (None, gpu):
        desc, texels, amin = itw.load_dds(f.tobytes(), device=device)
        assert (desc.width, desc.height, desc.mip_levels, desc.dxgi_format, desc.is_cubemap) == (16, 16, 5, 96, 1)      # the descriptor still says 96
        assert len(texels) == 30 and amin == [0x3C00] * 30
        for i, wimg in enumerate(want):
            assert np.array_equal(to_np(texels[i]), wimg), i
    # a file with mips and no cube
    f2 = itw.dds_file("bc6h_sf16", 16, 16, levels[:5], mip_levels=5)
    _, texels, amin = itw.load_dds(f2.tobytes())
    assert all(np.array_equal(t, wimg) for t, wimg in zip(texels, want[:5])) and amin == [0x3C00] * 5
    # examples/encode_dds --decode opens it the same way
    path, raw = tmp_path / "cube.dds", tmp_path / "cube.raw"
    f.tofile(path)
    r = subprocess.run([EXE, "--decode", str(path), str(raw)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(raw, dtype=np.uint16), np.concatenate([wimg.reshape(-1) for wimg in want]))
    assert r.stdout.splitlines()[0] == "image 0: 16 16 min_alpha 15360"
    ppm = tmp_path / "view.ppm"
    r = subprocess.run([EXE, "--preview", str(path), "0", str(ppm), "16", "16", "0", "0", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    shown = np.fromfile(ppm, dtype=np.uint8)[-16 * 16 * 3:].reshape(16, 16, 3)
    assert np.array_equal(shown, _preview.viewport(want[0], 16, 16, 0, 0, 1.0, 0, 0, 1.0))
    # itwDecodeBlocks(96, ...) on the same payload still gives the unsigned bytes
    out = np.full((16, 16, 4), SENTINEL, dtype=np.uint16)
    assert itw.lib().itwDecodeBlocks(96, levels[0].ctypes.data, 16, 16, out.ctypes.data, 128, None) == 0
    unsigned = image(H.model(levels[0], signed=False)["texels"], 16, 16)
    assert np.array_equal(out, unsigned) and np.array_equal(out, itw.decode("bc6h", levels[0], 16, 16)) and not np.array_equal(out, want[0])


# ---- 7. graph capture ------------------------------------------------------------------------------------------------------------------------

def test_captured_decode_and_measure_replay_to_the_same_bytes(itw, gpu, rec):
    import torch
    blocks, texels, modes, _ = rec["constructed"]
    w, h = LAYOUT["constructed"]
    decoded = image(texels, w, h)
    src = two_signed_source(decoded, 9)
    want = expected_stats(decoded, modes, src)[0]
    d_blocks, d_src = torch.from_numpy(blocks.copy()).to(gpu), torch.from_numpy(src.view(np.int16)).to(gpu)
    out = torch.zeros((h, w, 4), dtype=torch.int16, device=gpu)
    d_modes = torch.zeros(modes.size, dtype=torch.int32, device=gpu)
    amin = torch.zeros(1, dtype=torch.int32, device=gpu)
    stats = torch.zeros(C.sizeof(itw.ErrorStats), dtype=torch.uint8, device=gpu)
    surf = itw.RgbaSurface(out.data_ptr(), w, h, w * 8)
    L = itw.lib()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        L.itwSetStream(torch.cuda.current_stream().cuda_stream)
        assert L.itwDecodeImage(H.FORMAT, d_blocks.data_ptr(), C.byref(surf), d_modes.data_ptr(), amin.data_ptr()) == 0
        itw.measure_async(KEY, d_blocks, d_src, stats)
    torch.cuda.synchronize()
    for t in (out, d_modes, amin, stats):
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(to_np(out), decoded) and np.array_equal(d_modes.cpu().numpy(), modes) and int(amin.cpu()[0]) == 0x3C00
    assert itw.stats_from_tensor(stats).as_dict() == want
