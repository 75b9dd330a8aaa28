"""GPU, BC2 (ITW_FORMAT_BC2_UNORM[_SRGB], include/itw_dispatch.h): the encoder emits the bytes of the reference's D3DXEncodeBC2 as recorded in
tests/golden/bc2_ref.npz (tests/test_bc2_cpu.py holds reference == golden == model), through every entry point that takes the format; the
decode, measure, preview and load paths read what it writes.  Only the npz is read, never the reference.  Every comparison of encoded
bytes is equality."""
import ctypes as C

import numpy as np
import pytest

import _dxtex_bc2 as B2
import _preview
from _guarded import frozen, guarded
from conftest import first_mismatch

pytestmark = pytest.mark.gpu
BC2 = 0x83F2


def settings_of(itw, flags, ref=0.5):
    return itw.Bc1aSettings(float(ref), bool(flags & B2.DITHER_RGB), bool(flags & B2.DITHER_A), bool(flags & B2.UNIFORM))


def gpu_encode(itw, gpu, img, settings=None, fmt="bc2"):
    import torch
    out = itw.compress(fmt, torch.from_numpy(np.ascontiguousarray(img)).to(gpu), settings)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- 1. parity with D3DXEncodeBC2's recorded streams ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", B2.FLAG_SETS, ids=lambda f: "flags_%05x" % f)
def test_shared_content_vs_golden(itw, gpu, flags):
    """1 024 + 256 + 64 blocks; tests/test_bc2_cpu.py asserts what the dither does over them (raised, lowered, above 1, below 0)."""
    g = B2.golden()
    for name, img in B2.content().items():
        got = gpu_encode(itw, gpu, img, settings_of(itw, flags))
        want = g[B2.golden_key(name, flags)]
        assert got.size == want.size
        assert first_mismatch(got, want, 16) is None, (name, hex(flags), first_mismatch(got, want, 16))


def test_null_settings_are_the_explicit_defaults_srgb_only_labels_and_alpha_ref_is_not_read(itw, gpu):
    img = B2.content()["boundary"]
    a = gpu_encode(itw, gpu, img, None)
    assert np.array_equal(a, B2.golden()[B2.golden_key("boundary", 0)])
    assert np.array_equal(a, gpu_encode(itw, gpu, img, itw.Bc1aSettings()))
    assert np.array_equal(a, gpu_encode(itw, gpu, img, itw.Bc1aSettings(), fmt="bc2_srgb"))
    for ref in (0.0, 1.0, 1.5, -2.0):                       # BC2 has no colour key
        assert np.array_equal(a, gpu_encode(itw, gpu, img, itw.Bc1aSettings(ref)))
    d = gpu_encode(itw, gpu, img, itw.Bc1aSettings(1.5, dither_a=True))
    assert np.array_equal(d, B2.golden()[B2.golden_key("boundary", B2.DITHER_A)])


# ---- 2. sizes --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", B2.SIZES)
@pytest.mark.parametrize("flags", B2.SIZE_FLAGS)
def test_partial_blocks_take_the_directxtex_fill(itw, gpu, h, w, flags):
    img = B2.size_image(h, w)
    want = B2.golden()[B2.size_key(h, w, flags)]
    assert want.size == ((h + 3) // 4) * ((w + 3) // 4) * 16
    got = gpu_encode(itw, gpu, img, settings_of(itw, flags))                                   # device pointers
    assert first_mismatch(got, want, 16) is None, first_mismatch(got, want, 16)
    ok, host = itw.compress_image("bc2", img, settings=settings_of(itw, flags))              # host pointers
    assert ok and np.array_equal(host, want)


# ---- 3. pointer kinds, strides, guard bands --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src_dev,dst_dev", [(False, False), (True, True), (True, False), (False, True)])
@pytest.mark.parametrize("pitch,offset", [(300, 4), (304, 0)], ids=["pitch300_dword_loads", "pitch304_16B_aligned"])
def test_pointer_kinds_strides_and_guard_bands(itw, gpu, src_dev, dst_dev, pitch, offset):
    """A 61 x 75 view (300 bytes of texels per row) inside a larger allocation: rows 300 B apart at an address 4 past a multiple of 16 (the
    dword loads) and 304 B apart on one (the 16-byte loads); the target between two guard bands; the source unchanged."""
    h, w = 61, 75
    img = B2.size_image(h, w)
    want = B2.golden()[B2.size_key(h, w, 0)]
    src = frozen(img, row_pad=pitch - 4 * w, device=gpu if src_dev else None, align=16, offset=offset)
    assert src.stride == pitch and (src.ptr % 16 == 0) == (offset == 0)
    dst = guarded(want.size, device=gpu if dst_dev else None)
    surf = itw.RgbaSurface(src.ptr, w, h, pitch)
    s = itw.Bc1aSettings()
    assert itw.lib().itwCompressImageSlicedEx(C.byref(surf), dst.ptr, ((w + 3) // 4) * 16, BC2, C.cast(C.byref(s), C.c_void_p), 1 << 40, None, None), itw.last_error()
    assert np.array_equal(dst.host(), want)
    dst.check("BC2 target")
    src.check("BC2 source")


def test_slices_with_progress_give_the_one_slice_stream(itw, gpu):
    """256 x 256 in 16 slices of 4096 texels from pageable host memory."""
    img = np.tile(B2.content()["boundary"], (2, 2, 1))
    one = gpu_encode(itw, gpu, img)
    seen = []
    ok, out = itw.compress_image("bc2", img, slice_pixels=4096, progress=lambda i, n, u: (seen.append((i, n)), True)[1], settings=itw.Bc1aSettings())
    assert ok and np.array_equal(out, one) and seen == [(i, 16) for i in range(1, 16)]
    assert np.array_equal(one.reshape(64, 64, 16)[:32, :32], B2.golden()[B2.golden_key("boundary", 0)].reshape(32, 32, 16))


# ---- 4. chains -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_chain_of_a_16x16_cube_with_full_mips(itw, gpu, on_device):
    import torch
    images = [B2.cutout(16 >> l, 16 >> l, seed=10 * f + l) for f in range(6) for l in range(5)]          # 16 .. 1, face major
    s = itw.Bc1aSettings(dither_a=True, dither_rgb=True)
    want = np.concatenate([gpu_encode(itw, gpu, im, s) for im in images])                                 # each image: the single-image call
    assert itw.chain_bytes("bc2", images) == want.size == 6 * (16 + 4 + 1 + 1 + 1) * 16
    src = [torch.from_numpy(im).to(gpu) for im in images] if on_device else images
    seen = []
    ok, out = itw.compress_chain("bc2", src, settings=s, progress=lambda i, n, u: (seen.append(i), True)[1])
    got = out.cpu().numpy() if on_device else out
    assert ok and seen == list(range(1, len(images) + 1))
    assert first_mismatch(got, want, 16) is None, first_mismatch(got, want, 16)


@pytest.mark.parametrize("opts", [{}, {"srgb": True}, {"alpha_coverage": 128}, {"srgb": True, "alpha_coverage": 128}],
                         ids=["plain", "srgb", "coverage128", "srgb_coverage128"])
def test_mipped_64x64_is_the_chain_of_the_generated_levels(itw, gpu, opts):
    base = B2.cutout(64, 64, seed=3)
    s = itw.Bc1aSettings(dither_a=True)
    ok, blocks = itw.compress_mipped("bc2", base, settings=s, **opts)
    assert ok
    chain = itw.generate_mips(base, **opts)
    assert len(chain) == 7 and blocks.size == itw.chain_bytes("bc2", [lv.shape[:2] for lv in chain])
    want = np.concatenate([gpu_encode(itw, gpu, np.ascontiguousarray(lv), s) for lv in chain])
    assert np.array_equal(blocks, want)
    if opts:
        assert not np.array_equal(blocks, itw.compress_mipped("bc2", base, settings=s)[1])             # the option reached the generation


# ---- 5. decode -------------------------------------------------------------------------------------------------------------------------

def _tiles(img):
    h, w = img.shape[:2]
    return img.reshape(h // 4, 4, w // 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(-1, 16, 4)


def test_decode_of_constructed_blocks(itw, gpu):
    """Every nibble value in every position, endpoints in both orders and equal, all four indices (tests/_dxtex_bc2.py:
    decode_test_blocks).  Alpha equals the recorded D3DXDecodeBC2 exactly; colour lies within the 1.5 codes tests/test_reference_codecs.py
    allows BC1 / BC3 (two definitions of one block) and equals the BC3 decode of the same colour words; index 3 with c0 <= c1 is not black."""
    import torch
    g = B2.golden()
    blocks, ref = g["decode.blocks"], g["decode.ref"]
    stream = blocks.reshape(-1)
    dec = itw.decode_image("bc2", stream, (4, 256))                     # 64 blocks side by side
    ours = _tiles(dec)
    assert np.array_equal(dec, B2.np_decode(stream, 4, 256))
    assert np.array_equal(np.rint(ref[..., 3] * 255.0).astype(np.uint8), ours[..., 3])
    assert np.array_equal(ours[..., 3] % 17, np.zeros_like(ours[..., 3]))
    for k in range(16):                                                 # every nibble value in every position
        assert np.array_equal(ours[k, :, 3], ((np.arange(16) + k) & 15) * 17)
    assert np.abs(ref[..., :3] * 255.0 - ours[..., :3].astype(np.float32)).max() <= 1.5
    # the same colour words under BC3's alpha block
    as_bc3 = blocks.copy()
    as_bc3[:, :8] = np.array([255, 255, 0, 0, 0, 0, 0, 0], np.uint8)
    bc3 = _tiles(itw.decode_image("bc3", as_bc3.reshape(-1), (4, 256)))
    assert np.array_equal(bc3[..., :3], ours[..., :3])
    # c0 < c1 (k % 3 == 1): a BC1 decoder shows index 3 as transparent black; BC2 shows the fourth colour
    bc1 = _tiles(itw.decode_image("bc1", np.ascontiguousarray(blocks[:, 8:]).reshape(-1), (4, 256)))
    for k in range(1, 48, 3):
        idx3 = ((np.arange(16) + k) & 3) == 3
        assert (bc1[k, idx3] == 0).all() and ours[k, idx3, :3].any() and not np.array_equal(bc1[k, idx3, :3], ours[k, idx3, :3]), k
    # bc2_srgb, device pointers, the older entry point, modes
    assert np.array_equal(itw.decode_image("bc2_srgb", stream, (4, 256)), dec)
    assert np.array_equal(itw.decode("bc2", stream, 256, 4), dec)
    t, modes, amin = itw.decode_image("bc2", torch.from_numpy(stream.copy()).to(gpu), (4, 256), want_modes=True, want_min_alpha=True)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), dec) and not modes.cpu().numpy().any() and (int(amin.cpu()[0]) & 0xFFFFFFFF) == 0


def test_decode_chain_with_odd_sizes_tail_mips_and_minimum_alpha(itw, gpu):
    rng = np.random.default_rng(9)
    sizes = [(61, 75), (30, 37), (15, 18), (7, 9), (3, 4), (1, 2), (1, 1), (5, 3)]
    streams, floors = [], [0, 17, 34, 255, 119, 0, 238, 51]
    for (h, w), lo in zip(sizes, floors):
        n = ((h + 3) // 4) * ((w + 3) // 4)
        b = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        nib = rng.integers(lo // 17, 16, (n, 16))                      # alpha nibbles >= the image's floor
        nib[0, 0] = lo // 17                                           # ... which texel (0, 0) has
        b[:, :8] = (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)
        streams.append(b.reshape(-1))
    payload = np.concatenate(streams)
    texels, amin = itw.decode_chain("bc2", payload, sizes, want_min_alpha=True)
    at = 0
    for i, ((h, w), st) in enumerate(zip(sizes, streams)):
        want = B2.np_decode(st, h, w)
        assert np.array_equal(texels[i], want), (i, h, w)
        assert int(amin[i]) == int(want[..., 3].min()) == floors[i], (i, int(amin[i]), floors[i])
        assert np.array_equal(itw.decode_image("bc2", st, (h, w)), want) and np.array_equal(itw.decode("bc2", st, w, h), want)
        at += st.size
    assert at == payload.size == itw.chain_bytes("bc2", sizes)


# ---- 6. measure ------------------------------------------------------------------------------------------------------------------------

def _expect(itw, fmt, blocks, src):
    h, w = src.shape[:2]
    H, W = (h + 3) // 4 * 4, (w + 3) // 4 * 4
    dec = B2.np_decode(blocks, H, W)
    d = src.astype(np.int64) - dec[:h, :w].astype(np.int64)
    sq = d * d
    per_texel = np.zeros((H, W), dtype=np.int64)
    per_texel[:h, :w] = sq.sum(axis=2)
    bmap = per_texel.reshape(H // 4, 4, W // 4, 4).sum(axis=(1, 3)).reshape(-1)
    nb = (H // 4) * (W // 4)
    return {"dxgi_format": itw.DXGI_FORMAT[fmt], "width": w, "height": h, "reserved_blocks": 0, "blocks": nb,
            "sse": [int(v) for v in sq.sum(axis=(0, 1))], "max_abs": [int(v) for v in np.abs(d).max(axis=(0, 1))],
            "worst_block_sse": int(bmap.max()), "worst_block": int(np.argmax(bmap)), "mode_hist": [nb] + [0] * 15}, bmap


def test_measure_of_an_encoded_61x75_image(itw, gpu):
    import torch
    img = B2.size_image(61, 75)
    stream = B2.golden()[B2.size_key(61, 75, 0)]
    want, bmap = _expect(itw, "bc2", stream, img)
    assert want["sse"][3] > 0 and want["max_abs"][3] <= 8               # 4-bit alpha: at most half a step of 17 off
    st, got_map = itw.measure("bc2", stream, img, want_block_map=True)
    assert st.as_dict() == want and np.array_equal(got_map, bmap.astype(np.uint64))
    assert st.mse() == sum(want["sse"]) / (61 * 75 * 4.0)               # own channels: RGBA
    st_d = itw.measure("bc2_srgb", torch.from_numpy(stream.copy()).to(gpu), torch.from_numpy(img).to(gpu))
    assert st_d.as_dict() == dict(want, dxgi_format=itw.DXGI_FORMAT["bc2_srgb"])
    assert st.psnr() == st_d.psnr() > 20.0


def test_measure_chain_excludes_padding(itw, gpu):
    images = [B2.size_image(h, w) for h, w in ((61, 75), (5, 3), (1, 1), (4, 4))]
    streams = [B2.golden()[B2.size_key(im.shape[0], im.shape[1], 0)] for im in images]
    res = itw.measure_chain("bc2", np.concatenate(streams), images)
    assert len(res) == 4
    for st, im, s in zip(res, images, streams):
        assert st.as_dict() == _expect(itw, "bc2", s, im)[0], im.shape


# ---- 7. preview ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("zoom", [1.0, 3.0])
def test_preview_of_a_128x128_stream(itw, gpu, zoom, device):
    import torch
    stream = B2.golden()[B2.golden_key("boundary", B2.DITHER_A)]
    texels = B2.np_decode(stream, 128, 128)
    for channels, x, y in (("rgb", 0, 0), ("rgba", -3, 5), ("a", 7, -2)):
        view = dict(view_w=70, view_h=50, x=x, y=y, zoom=zoom, channels=channels, matte=0x00336699)
        if device:
            got = itw.preview("bc2", torch.from_numpy(stream.copy()).to(gpu), 128, 128, **view)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
        else:
            got = itw.preview("bc2", stream, 128, 128, **view)
        options = sum({"r": 4, "g": 8, "b": 16, "a": 32}[c] for c in channels)
        want = _preview.viewport(texels, 70, 50, x, y, zoom, options, 0x00336699, 1.0)
        assert got.shape == want.shape and np.array_equal(got, want), (channels, zoom, np.argwhere((got != want).any(axis=2))[:4])


# ---- 8. the load path ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key,header", [("bc2", 128), ("bc2_srgb", 148)])
def test_load_dds_of_a_mipped_cube(itw, gpu, key, header):
    images = [B2.cutout(16 >> l, 16 >> l, seed=10 * f + l) for f in range(6) for l in range(5)]
    ok, blocks = itw.compress_chain(key, images)
    assert ok
    sizes = [16 * ((im.shape[0] + 3) // 4) * ((im.shape[1] + 3) // 4) for im in images]
    levels = np.split(blocks, np.cumsum(sizes)[:-1])
    f = itw.dds_file(key, 16, 16, levels, mip_levels=5, cubemap=True)
    assert f.size == header + blocks.size and f[84:88].tobytes() == (b"DXT3" if key == "bc2" else b"DX10")
    for device in (None, gpu):
        desc, texels, amin = itw.load_dds(f.tobytes(), device=device)
        assert (desc.width, desc.height, desc.mip_levels, desc.dxgi_format, desc.is_cubemap) == (16, 16, 5, itw.DXGI_FORMAT[key], 1)
        assert len(texels) == 30
        for i, (im, lv) in enumerate(zip(images, levels)):
            t = texels[i] if device is None else texels[i].cpu().numpy()
            want = B2.np_decode(lv, im.shape[0], im.shape[1])
            assert np.array_equal(t, want), i
            assert amin[i] == int(want[..., 3].min())
            assert np.abs(t[..., 3].astype(int) - im[..., 3].astype(int)).max() <= 8          # it is the image that was encoded
