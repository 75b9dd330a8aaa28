"""GPU, BC3 by DirectXTex's encoder (ITW_FORMAT_BC3_DXTEX[_SRGB], include/itw_dispatch.h): the encoder emits the bytes of the reference's
D3DXEncodeBC3 as recorded in tests/golden/bc3_dxtex_ref.npz (tests/test_bc3_dxtex_cpu.py holds reference == golden == model), through every
entry point that takes the codes; images the recording does not hold are compared with the numpy model of tests/_dxtex_bc3.py, which that
file pins to the reference.  The decode, measure and preview entry points read the codes as 77 / 78.  Only the npz is read, never the
reference.  Every comparison of encoded bytes is equality."""
import ctypes as C

import numpy as np
import pytest

import _dxtex_bc3 as B3
import _stream_order as so
from _dxtex_bc2 import cutout
from _dxtex_snorm import block_texels
from _guarded import frozen, guarded
from conftest import first_mismatch

pytestmark = pytest.mark.gpu
BC3DX = 0x83F3


def settings_of(itw, flags, ref=0.5):
    return itw.Bc1aSettings(float(ref), bool(flags & B3.DITHER_RGB), bool(flags & B3.DITHER_A), bool(flags & B3.UNIFORM))


def gpu_encode(itw, gpu, img, settings=None, fmt="bc3_dxtex"):
    import torch
    out = itw.compress(fmt, torch.from_numpy(np.ascontiguousarray(img)).to(gpu), settings)
    torch.cuda.synchronize()
    return out.cpu().numpy()


_models = {}


def model_stream(img, flags=0):
    """The reference's stream of an image the recording does not hold, by the model; computed once per image and flag set."""
    img = np.ascontiguousarray(img)
    key = (img.shape, img.tobytes(), flags)
    if key not in _models:
        _models[key] = B3.model(block_texels(img), flags)[0].reshape(-1)
    return _models[key]


# ---- 1. parity with D3DXEncodeBC3's recorded streams ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", B3.FLAG_SETS, ids=lambda f: "flags_%05x" % f)
def test_shared_content_vs_golden(itw, gpu, flags):
    """1 024 + 256 + 128 blocks from device pointers; tests/test_bc3_dxtex_cpu.py asserts which branches of the alpha half they take."""
    g = B3.golden()
    for name, img in B3.content().items():
        got = gpu_encode(itw, gpu, img, settings_of(itw, flags))
        want = g[B3.golden_key(name, flags)]
        assert got.size == want.size
        assert first_mismatch(got, want, 16) is None, (name, hex(flags), first_mismatch(got, want, 16))


def test_null_settings_are_the_explicit_defaults_srgb_only_labels_and_alpha_ref_is_not_read(itw, gpu):
    img = B3.content()["boundary"]
    g = B3.golden()
    a = gpu_encode(itw, gpu, img, None)
    assert np.array_equal(a, g[B3.golden_key("boundary", 0)])
    assert np.array_equal(a, gpu_encode(itw, gpu, img, itw.Bc1aSettings()))
    assert np.array_equal(a, gpu_encode(itw, gpu, img, itw.Bc1aSettings(), fmt="bc3_dxtex_srgb"))
    for ref in (0.0, 1.0, 1.5, -2.0):                       # BC3 has no colour key
        assert np.array_equal(a, gpu_encode(itw, gpu, img, itw.Bc1aSettings(ref)))
    assert np.array_equal(gpu_encode(itw, gpu, img, itw.Bc1aSettings(1.5, dither_a=True)), g[B3.golden_key("boundary", B3.DITHER_A)])
    # 77 keeps its encoder: kernel.ispc's stream of the same texels is another stream
    assert not np.array_equal(a, gpu_encode(itw, gpu, img, None, fmt="bc3"))


# ---- 2. sizes --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", B3.SIZES)
@pytest.mark.parametrize("flags", B3.SIZE_FLAGS)
def test_partial_blocks_take_the_directxtex_fill(itw, gpu, h, w, flags):
    img = B3.size_image(h, w)
    want = B3.golden()[B3.size_key(h, w, flags)]
    assert want.size == ((h + 3) // 4) * ((w + 3) // 4) * 16
    got = gpu_encode(itw, gpu, img, settings_of(itw, flags))                                   # device pointers
    assert first_mismatch(got, want, 16) is None, first_mismatch(got, want, 16)
    ok, host = itw.compress_image("bc3_dxtex", img, settings=settings_of(itw, flags))         # host pointers
    assert ok and np.array_equal(host, want)


@pytest.mark.parametrize("h,w", [(4, 1028), (1, 1)], ids=["257_blocks_one_past_a_workgroup", "one_texel"])
def test_one_block_past_a_workgroup_and_a_single_texel(itw, gpu, h, w):
    img = cutout(h, w, seed=77)
    for flags in B3.SIZE_FLAGS:
        want = model_stream(img, flags)
        assert want.size == ((h + 3) // 4) * ((w + 3) // 4) * 16
        got = gpu_encode(itw, gpu, img, settings_of(itw, flags))
        assert first_mismatch(got, want, 16) is None, (hex(flags), first_mismatch(got, want, 16))
        ok, host = itw.compress_image("bc3_dxtex", img, settings=settings_of(itw, flags))
        assert ok and np.array_equal(host, want)


# ---- 3. pointer kinds, strides, guard bands: the load and store variants --------------------------------------------------------------

@pytest.mark.parametrize("src_dev,dst_dev", [(False, False), (True, True), (True, False), (False, True)])
@pytest.mark.parametrize("pitch,offset,dst_offset", [(300, 4, 0), (304, 0, 0), (304, 0, 4), (300, 4, 4)],
                         ids=["pitch300_dword_loads", "pitch304_16B_loads", "target_plus_4_dword_stores", "dword_loads_and_stores"])
def test_pointer_kinds_strides_and_guard_bands(itw, gpu, src_dev, dst_dev, pitch, offset, dst_offset):
    """A 61 x 75 view (300 bytes of texels per row) inside a guarded canvas: rows 300 B apart at an address 4 past a multiple of 16 (the
    dword loads) and 304 B apart on one (the 16-byte loads); the target between two guard bands, on a multiple of 16 (one 16-byte store
    per block) and 4 past one (four dword stores); the source unchanged."""
    h, w = 61, 75
    img = B3.size_image(h, w)
    want = B3.golden()[B3.size_key(h, w, 0)]
    src = frozen(img, row_pad=pitch - 4 * w, device=gpu if src_dev else None, align=16, offset=offset)
    assert src.stride == pitch and (src.ptr % 16 == 0) == (offset == 0)
    dst = guarded(want.size, device=gpu if dst_dev else None, offset=dst_offset)
    assert dst.ptr % 16 == dst_offset
    surf = itw.RgbaSurface(src.ptr, w, h, pitch)
    s = itw.Bc1aSettings()
    assert itw.lib().itwCompressImageSlicedEx(C.byref(surf), dst.ptr, ((w + 3) // 4) * 16, BC3DX, C.cast(C.byref(s), C.c_void_p), 1 << 40, None, None), itw.last_error()
    assert np.array_equal(dst.host(), want)
    dst.check("BC3_DXTEX target")
    src.check("BC3_DXTEX source")


def test_a_target_inside_a_dds_payload_behind_a_148_byte_header(itw, gpu):
    """The stream written where a DX10 file holds it: 148 bytes into a device buffer, 4 past a multiple of 16; the file around it stays."""
    import torch
    img = B3.content()["strip"]
    want = B3.golden()[B3.golden_key("strip", B3.DITHER_A)]
    f = itw.dds_file("bc3_dxtex_srgb", 128, 32, [np.zeros(want.size, np.uint8)])
    assert f.size == 148 + want.size
    dev = torch.from_numpy(np.concatenate([f, np.full(64, 0xA5, np.uint8)])).to(gpu)
    t = torch.from_numpy(img).to(gpu)
    surf = itw.RgbaSurface(t.data_ptr(), 128, 32, 512)
    s = itw.Bc1aSettings(dither_a=True)
    assert (dev.data_ptr() + 148) % 16 == 4
    assert itw.lib().itwCompressImageSlicedEx(C.byref(surf), dev.data_ptr() + 148, 32 * 16, 0x8C4F, C.cast(C.byref(s), C.c_void_p), 1 << 40, None, None), itw.last_error()
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    assert np.array_equal(got[:148], f[:148]) and np.array_equal(got[148:-64], want) and (got[-64:] == 0xA5).all()
    assert np.array_equal(got[:-64], itw.dds_file("bc3_srgb", 128, 32, [want]))


# ---- 4. slices -------------------------------------------------------------------------------------------------------------------------

def test_slices_with_progress_and_abort_give_the_one_call_stream(itw, gpu):
    """256 x 256 in 16 slices of 4096 texels from pageable host memory: the pipeline's stream is the one-slice stream, whose top left is
    the recording; a callback that stops at slice 2 leaves the first slices' bytes and returns False."""
    img = np.tile(B3.content()["boundary"], (2, 2, 1))
    one = gpu_encode(itw, gpu, img)
    assert np.array_equal(one.reshape(64, 64, 16)[:32, :32].reshape(-1), B3.golden()[B3.golden_key("boundary", 0)])
    seen = []
    ok, out = itw.compress_image("bc3_dxtex", img, slice_pixels=4096, progress=lambda i, n, u: (seen.append((i, n)), True)[1], settings=itw.Bc1aSettings())
    assert ok and np.array_equal(out, one) and seen == [(i, 16) for i in range(1, 16)]
    itw.lib().itwSetSliceWindow(1)                      # one slice per window, so the abort lands where it is asked
    try:
        stop = []
        ok, part = itw.compress_image("bc3_dxtex", img, slice_pixels=4096, progress=lambda i, n, u: (stop.append(i), i < 2)[1], settings=itw.Bc1aSettings())
    finally:
        itw.lib().itwSetSliceWindow(0)
    assert not ok and stop == [1, 2]
    n = (256 // 4 // 16 * 2) * 64 * 16                  # block rows of slices 0 and 1
    assert np.array_equal(part[:n], one[:n])


# ---- 5. chains -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("shape", ["mips_20x12", "cube_16"])
def test_chain_images_are_the_references_streams(itw, gpu, on_device, shape):
    import torch
    if shape == "cube_16":
        images = [cutout(16 >> l, 16 >> l, seed=10 * f + l) for f in range(6) for l in range(5)]          # 16 .. 1, face major
    else:
        images = [cutout(max(1, 12 >> l), max(1, 20 >> l), seed=40 + l) for l in range(5)]                # 20 x 12 .. 1 x 1
    flags = B3.DITHER_A | B3.DITHER_RGB
    s = settings_of(itw, flags)
    want = np.concatenate([model_stream(im, flags) for im in images])
    assert itw.chain_bytes("bc3_dxtex", images) == want.size == itw.chain_bytes("bc2", images)
    src = [torch.from_numpy(im).to(gpu) for im in images] if on_device else images
    seen = []
    ok, out = itw.compress_chain("bc3_dxtex", src, settings=s, progress=lambda i, n, u: (seen.append(i), True)[1])
    got = out.cpu().numpy() if on_device else out
    assert ok and seen == list(range(1, len(images) + 1))
    assert first_mismatch(got, want, 16) is None, first_mismatch(got, want, 16)


@pytest.mark.parametrize("opts", [{"alpha_coverage": 128}, {"srgb": True, "alpha_coverage": 128}, {}], ids=["coverage128", "srgb_coverage128", "plain"])
def test_mipped_64x64_is_the_chain_of_the_generated_levels_and_the_dds_payload(itw, gpu, opts):
    base = cutout(64, 64, seed=3)
    s = itw.Bc1aSettings(dither_a=True)
    ok, blocks = itw.compress_mipped("bc3_dxtex", base, settings=s, **opts)
    assert ok
    chain = itw.generate_mips(base, **opts)
    assert len(chain) == 7 and blocks.size == itw.chain_bytes("bc3_dxtex", [lv.shape[:2] for lv in chain])
    levels = [model_stream(lv, B3.DITHER_A) for lv in chain]
    assert first_mismatch(blocks, np.concatenate(levels), 16) is None, first_mismatch(blocks, np.concatenate(levels), 16)
    if opts:
        assert not np.array_equal(blocks, itw.compress_mipped("bc3_dxtex", base, settings=s)[1])      # the option reached the generation
    f = itw.dds_file("bc3_dxtex", 64, 64, levels, mip_levels=7)
    assert f[84:88].tobytes() == b"DXT5" and np.array_equal(f[128:], blocks)
    desc, texels, _ = itw.load_dds(f.tobytes())
    assert (desc.width, desc.height, desc.mip_levels, desc.dxgi_format) == (64, 64, 7, 77) and len(texels) == 7
    assert np.abs(texels[0][..., 3].astype(int) - chain[0][..., 3].astype(int)).max() <= 40            # it is the image that was encoded


# ---- 6. the stream read back: 0x83F3 is 77 on the decode side ---------------------------------------------------------------------------

def test_decode_measure_and_preview_read_the_codes_as_77_and_78(itw, gpu):
    import torch
    images = [B3.size_image(h, w) for h, w in ((61, 75), (5, 3), (1, 1), (4, 4))]
    streams = [B3.golden()[B3.size_key(im.shape[0], im.shape[1], 0)] for im in images]
    payload = np.concatenate(streams)
    sizes = [im.shape[:2] for im in images]
    for key, same in (("bc3_dxtex", "bc3"), ("bc3_dxtex_srgb", "bc3_srgb")):
        a, amin_a = itw.decode_chain(key, payload, sizes, want_min_alpha=True)
        b, amin_b = itw.decode_chain(same, payload, sizes, want_min_alpha=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and list(amin_a) == list(amin_b)
        ra, rb = itw.measure_chain(key, payload, images), itw.measure_chain(same, payload, images)
        assert [s.as_dict() for s in ra] == [s.as_dict() for s in rb] and ra[0].as_dict()["dxgi_format"] == itw.DXGI_FORMAT[same]
        st = itw.measure(key, torch.from_numpy(streams[0].copy()).to(gpu), torch.from_numpy(images[0]).to(gpu))
        assert st.as_dict() == ra[0].as_dict() and st.as_dict()["sse"][3] > 0
        assert np.array_equal(itw.decode_image(key, streams[0], (61, 75)), a[0])
        # itwDecodeBlocks keeps 77's own rule under the synonym: whole blocks only (BC3 is one of kernel.ispc's formats there)
        assert np.array_equal(itw.decode(key, streams[3], 4, 4), a[3]) and np.array_equal(itw.decode("bc3", streams[3], 4, 4), a[3])
        for fmt in (key, "bc3"):
            with pytest.raises(ValueError):
                itw.decode(fmt, streams[0], 75, 61)
        for zoom, channels in ((1.0, "rgba"), (3.0, "a")):
            view = dict(view_w=70, view_h=50, x=-3, y=5, zoom=zoom, channels=channels, matte=0x00336699)
            assert np.array_equal(itw.preview(key, streams[0], 75, 61, **view), itw.preview(same, streams[0], 75, 61, **view))
    # it is the image that was encoded: 8 alpha levels over at most the whole range
    assert np.abs(a[0][..., 3].astype(int) - images[0][..., 3].astype(int)).max() <= 40


# ---- 7. stream order --------------------------------------------------------------------------------------------------------------------

def test_the_sliced_and_chain_calls_keep_stream_order_with_the_callers_work(itw, gpu):
    """tests/_stream_order.py's synchronous scheme (sequences B and C): the caller's stream is busy, the copy that produces the call's device
    texels is queued behind that work, and the call must read the texels the copy leaves, not those before it: the result is the
    recorded stream of the content the copy brings."""
    import torch
    g = B3.golden()
    b = B3.content()["boundary"]
    contents = [[np.ascontiguousarray(b[::-1])], [b]]
    want = [g[B3.golden_key("boundary", B3.DITHER_A)]]
    s = itw.Bc1aSettings(dither_a=True)

    def sliced(to_host):
        def call(srcs):
            out = np.full(want[0].size, so.PRE, np.uint8) if to_host else torch.full((want[0].size,), so.PRE, dtype=torch.uint8, device=gpu)
            ok, _ = so._window_of_two(itw, lambda: itw.compress_image("bc3_dxtex", srcs[0], slice_pixels=2048, out=out, settings=s))
            assert ok
            return [out]
        return call

    def chain(srcs):
        ok, out = itw.compress_chain("bc3_dxtex", srcs, settings=s)
        assert ok
        return [out]
    delay = so.Delay(torch, gpu)
    S = torch.cuda.Stream(gpu)
    delay(S)
    torch.cuda.synchronize()
    env = so.Env(itw, None, gpu, torch, delay, S, so.Report())
    try:
        so.run_sync("bc3_dxtex sliced -> device", so.SyncCase(contents, want, sliced(False)), env)
        so.run_sync("bc3_dxtex sliced -> host", so.SyncCase(contents, want, sliced(True)), env)
        so.run_sync("bc3_dxtex chain", so.SyncCase(contents, want, chain), env)
    finally:
        itw.lib().itwSetStream(None)
        torch.cuda.synchronize()
