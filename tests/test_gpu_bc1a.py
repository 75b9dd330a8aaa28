"""GPU, BC1 with 1-bit alpha (ITW_FORMAT_BC1A_UNORM[_SRGB], include/itw_dispatch.h): the encoder emits the bytes of the reference's own
D3DXEncodeBC1 (tests/_dxtex_bc1.py: oracle/_ref/libdxtex_bc_ref.so, BC.cpp compiled unmodified) and of its recorded streams
(tests/golden/bc1a_ref.npz), through every entry point that takes the format; the decode side reads the codes as 71 / 72.  Every comparison
of encoded bytes is equality."""
import ctypes as C

import numpy as np
import pytest

import _dxtex_bc1 as B
from _guarded import frozen, guarded
from conftest import first_mismatch

pytestmark = pytest.mark.gpu
BC1A = 0x83F1
ALL_T = np.array([0, 0, 255, 255, 255, 255, 255, 255], np.uint8)
_want = {}


def settings_of(itw, ref, flags):
    return itw.Bc1aSettings(float(ref), bool(flags & B.DITHER_RGB), bool(flags & B.DITHER_A), bool(flags & B.UNIFORM))


def want_stream(key, img, ref=0.5, flags=0):
    """The reference's stream for `img`, computed once per key and shared."""
    k = (key, float(ref), flags)
    if k not in _want:
        _want[k] = B.encode(img, ref, flags)
        _want[k].setflags(write=False)
    return _want[k]


def cutout(h, w, seed=7):
    """Cut-out content: smooth colour, an alpha plane of discs with soft rims (every alpha code occurs) and fully transparent / opaque areas."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.zeros((h, w, 4), dtype=np.uint8)
    img[..., 0] = (x * 255 / max(1, w - 1)).astype(np.uint8)
    img[..., 1] = (y * 255 / max(1, h - 1)).astype(np.uint8)
    img[..., 2] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    a = np.zeros((h, w), dtype=np.float32)
    for _ in range(6):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(4, max(5, min(h, w) / 3))
        a = np.maximum(a, np.clip((r - np.hypot(y - cy, x - cx)) / 3.0 + 0.5, 0, 1))
    img[..., 3] = np.rint(a * 255).astype(np.uint8)
    return img


def gpu_encode(itw, gpu, img, settings=None, fmt="bc1a"):
    import torch
    out = itw.compress(fmt, torch.from_numpy(np.ascontiguousarray(img)).to(gpu), settings)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- 1. parity with D3DXEncodeBC1 and its recorded streams -----------------------------------------------------------------------------

@pytest.mark.parametrize("flags", B.FLAG_SETS, ids=lambda f: "flags_%05x" % f)
def test_shared_content_vs_golden_and_reference(itw, gpu, flags):
    """1 024 + 256 blocks whose census (tests/test_bc1a_cpu.py) takes every branch of the source, 5 alpha_ref values per flag set."""
    g = B.golden()
    for name, img in B.content().items():
        for ref in B.ALPHA_REFS:
            got = gpu_encode(itw, gpu, img, settings_of(itw, ref, flags))
            want = g[B.golden_key(name, ref, flags)]
            assert got.size == want.size
            assert first_mismatch(got, want, 8) is None, (name, float(ref), hex(flags), first_mismatch(got, want, 8))
    # ... and the reference itself, where its library is present, on one configuration per flag set (the golden file is its recording)
    img = B.content()["strip"]
    assert np.array_equal(gpu_encode(itw, gpu, img, settings_of(itw, B.ALPHA_REFS[2], flags)), want_stream("strip", img, B.ALPHA_REFS[2], flags))


def test_null_settings_are_the_explicit_defaults_and_srgb_only_labels(itw, gpu):
    img = B.content()["boundary"]
    a = gpu_encode(itw, gpu, img, None)
    assert np.array_equal(a, gpu_encode(itw, gpu, img, itw.Bc1aSettings()))
    assert np.array_equal(a, gpu_encode(itw, gpu, img, itw.Bc1aSettings(0.5, False, False, False), fmt="bc1a_srgb"))
    assert np.array_equal(a, B.golden()[B.golden_key("boundary", 0.5, 0)])
    # alpha_ref > 1: every block is the transparent block; <= 0: nothing is transparent, whatever the value
    assert (gpu_encode(itw, gpu, img, itw.Bc1aSettings(1.5)).reshape(-1, 8) == ALL_T).all()
    assert np.array_equal(gpu_encode(itw, gpu, img, itw.Bc1aSettings(0.0)), gpu_encode(itw, gpu, img, itw.Bc1aSettings(-2.0)))


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (5, 3), (4, 4), (61, 75)])
@pytest.mark.parametrize("flags", [0, B.DITHER_RGB | B.DITHER_A])
def test_partial_blocks_take_the_directxtex_fill(itw, gpu, h, w, flags):
    img = cutout(h, w, seed=h * 100 + w)
    want = want_stream(("size", h, w), img, 0.5, flags)
    assert want.size == ((h + 3) // 4) * ((w + 3) // 4) * 8
    got = gpu_encode(itw, gpu, img, settings_of(itw, 0.5, flags))
    assert first_mismatch(got, want, 8) is None, first_mismatch(got, want, 8)
    ok, host = itw.compress_image("bc1a", img, settings=settings_of(itw, 0.5, flags))         # host pointers
    assert ok and np.array_equal(host, want)


# ---- 2. pointer kinds, strides, guard bands --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src_dev,dst_dev", [(False, False), (True, True), (True, False), (False, True)])
@pytest.mark.parametrize("pitch,offset", [(300, 4), (304, 0)], ids=["pitch300_dword_loads", "pitch304_16B_aligned"])
def test_pointer_kinds_strides_and_guard_bands(itw, gpu, src_dev, dst_dev, pitch, offset):
    """A 61 x 75 view (300 bytes of texels per row) inside a larger allocation: rows 300 B apart at an address 4 past a multiple of 16 (the
    dword loads) and 304 B apart on one (the 16-byte loads); the target between two guard bands; the source unchanged."""
    h, w = 61, 75
    img = cutout(h, w, seed=11)
    want = want_stream(("size", h, w, 11), img)
    src = frozen(img, row_pad=pitch - 4 * w, device=gpu if src_dev else None, align=16, offset=offset)
    assert src.stride == pitch and (src.ptr % 16 == 0) == (offset == 0)
    dst = guarded(want.size, device=gpu if dst_dev else None)
    surf = itw.RgbaSurface(src.ptr, w, h, pitch)
    s = itw.Bc1aSettings()
    assert itw.lib().itwCompressImageSlicedEx(C.byref(surf), dst.ptr, ((w + 3) // 4) * 8, BC1A, C.cast(C.byref(s), C.c_void_p), 1 << 40, None, None), itw.last_error()
    assert np.array_equal(dst.host(), want)
    dst.check("BC1A target")
    src.check("BC1A source")


def test_64_slices_with_progress_and_abort(itw, gpu):
    """512 x 512 in 64 slices of 4096 texels from pageable host memory: the pipeline's stream is the one-slice stream; a callback that stops
    at slice 2 leaves the first slices' bytes -- a prefix of that stream -- and returns False."""
    img = np.tile(B.content()["boundary"], (4, 4, 1))
    one = gpu_encode(itw, gpu, img)
    seen = []
    ok, out = itw.compress_image("bc1a", img, slice_pixels=4096, progress=lambda i, n, u: (seen.append((i, n)), True)[1], settings=itw.Bc1aSettings())
    assert ok and np.array_equal(out, one) and seen == [(i, 64) for i in range(1, 64)]
    itw.lib().itwSetSliceWindow(1)                      # one slice per window, so the abort lands where it is asked
    try:
        stop = []
        ok, part = itw.compress_image("bc1a", img, slice_pixels=4096, progress=lambda i, n, u: (stop.append(i), i < 2)[1], settings=itw.Bc1aSettings())
    finally:
        itw.lib().itwSetSliceWindow(0)
    assert not ok and stop == [1, 2]
    rows = 512 // 4 // 64 * 2                           # block rows of slices 0 and 1
    n = rows * 128 * 8
    assert np.array_equal(part[:n], one[:n])


# ---- 3. chains -------------------------------------------------------------------------------------------------------------------------

def chain_images():
    rng = np.random.default_rng(21)
    cube = [cutout(64 >> l, 64 >> l, seed=int(rng.integers(1 << 30))) for _ in range(6) for l in range(7)]        # 64 .. 1, face major
    odd = [cutout(h, w, seed=h + w) for h, w in ((61, 75), (3, 5), (1, 1), (130, 34))]
    return cube + odd


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_chain_of_a_cube_with_mips_and_odd_images(itw, gpu, on_device):
    import torch
    images = chain_images()
    s = itw.Bc1aSettings(B.ALPHA_REFS[2], dither_a=True)
    want = np.concatenate([want_stream(("chain", i), im, B.ALPHA_REFS[2], B.DITHER_A) for i, im in enumerate(images)])
    assert itw.chain_bytes("bc1a", images) == want.size
    src = [torch.from_numpy(im).to(gpu) for im in images] if on_device else images
    seen = []
    ok, out = itw.compress_chain("bc1a", src, settings=s, progress=lambda i, n, u: (seen.append(i), True)[1])
    got = out.cpu().numpy() if on_device else out
    assert ok and seen == list(range(1, len(images) + 1))
    assert first_mismatch(got, want, 8) is None, first_mismatch(got, want, 8)


def test_large_aligned_image_of_a_chain_is_encoded_in_place(itw, gpu):
    """An image of a window's worth of blocks (262 144) whose size is a multiple of 4 is not gathered: 2048 x 2048 of tiled content, then a
    small odd image behind it."""
    tile = B.content()["boundary"]
    big = np.tile(tile, (16, 16, 1))
    small = cutout(5, 3, seed=2)
    ok, out = itw.compress_chain("bc1a", [big, small])
    assert ok
    t = B.golden()[B.golden_key("boundary", 0.5, 0)].reshape(32, 32, 8)
    assert np.array_equal(out[:-16].reshape(512, 512, 8), np.tile(t, (16, 16, 1)))
    assert np.array_equal(out[-16:], want_stream("small53", small))


# ---- 4. the decode side: a BC1A stream is a BC1 stream ---------------------------------------------------------------------------------

def test_decode_measure_preview_take_the_codes_as_71(itw, gpu):
    img = B.content()["boundary"]
    stream = B.golden()[B.golden_key("boundary", 0.5, 0)]
    for new, old in (("bc1a", "bc1"), ("bc1a_srgb", "bc1_srgb")):
        a, ma = itw.decode_image(new, stream, (128, 128), want_modes=True)
        b, mb = itw.decode_image(old, stream, (128, 128), want_modes=True)
        assert np.array_equal(a, b) and np.array_equal(ma, mb)
        assert bytes(itw.measure(new, stream, img)) == bytes(itw.measure(old, stream, img))
        sa, sb = itw.measure_chain(new, stream, [img]), itw.measure_chain(old, stream, [img])
        assert bytes(sa[0]) == bytes(sb[0]) and int(sa[0].dxgi_format) == itw.DXGI_FORMAT[old]
        assert np.array_equal(itw.preview(new, stream, 128, 128, 96, 80, x=3, y=5, zoom=1.5, channels="rgba"),
                              itw.preview(old, stream, 128, 128, 96, 80, x=3, y=5, zoom=1.5, channels="rgba"))
    assert np.array_equal(itw.decode("bc1a", stream, 128, 128), itw.decode("bc1", stream, 128, 128))
    # odd sizes: the decode side pads to whole blocks whatever the format
    odd = cutout(61, 75, seed=11)
    s = want_stream(("size", 61, 75, 11), odd)
    assert np.array_equal(itw.decode_image("bc1a", s, (61, 75)), itw.decode_image("bc1", s, (61, 75)))


def test_device_decoder_against_the_references_decoder(itw, gpu):
    """D3DXDecodeBC1 on the encoded stream.  Alpha and the choice between the 3- and 4-colour palettes are exact: the reference's alpha is 0.0f
    or 1.0f, the device's 0 or 255, texel for texel.  Colour: DirectXTex expands 5:6:5 as c/31, c/63 and interpolates in float, the device
    decoder replicates bits and interpolates integers -- two definitions of the same block that tests/test_reference_codecs.py pins to
    within 1.5 codes of each other; the same bound here."""
    for name, img in B.content().items():
        stream = B.golden()[B.golden_key(name, 0.5, 0)]
        h, w = img.shape[:2]
        dec = itw.decode_image("bc1a", stream, (h, w))
        ours = dec.reshape(h // 4, 4, w // 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(-1, 16, 4)
        ref = B.decode(stream)
        assert np.array_equal(np.rint(ref[..., 3] * 255.0).astype(np.uint8), ours[..., 3])
        assert set(np.unique(ours[..., 3])) <= {0, 255}
        # a transparent texel is the source's a < 128 exactly (alpha_ref 0.5 lies between codes 127 and 128)
        src = B.block_texels(img)
        assert np.array_equal(ours[..., 3] == 0, src[..., 3] < 128)
        assert np.abs(ref[..., :3] * 255.0 - ours[..., :3].astype(np.float32)).max() <= 1.5


# ---- 5. what the feature exists for: cut-out textures keep their coverage through the encoder -------------------------------------------

@pytest.mark.parametrize("h,w", [(64, 64), (61, 75)])
@pytest.mark.parametrize("r", [1, 128, 255])
def test_mipped_cutout_keeps_the_reported_coverage(itw, gpu, h, w, r):
    """compress_mipped(..., alpha_coverage=r) rescales every level's alpha so that the share of texels with a >= r is kept; with
    alpha_ref = r * (1/255) the encoder makes exactly the texels with a < r transparent.  So per image the number of decoded texels with
    alpha 255 is the report's `covered`."""
    base = cutout(h, w, seed=r)
    s = itw.Bc1aSettings(alpha_ref=itw.Bc1aSettings.ref_of(r))
    ok, blocks, rows = itw.compress_mipped("bc1a", base, alpha_coverage=r, report=True, settings=s)
    assert ok
    n = itw.mip_levels(w, h)
    sizes = [(max(1, h >> l), max(1, w >> l)) for l in range(n)]
    assert len(rows) == n and blocks.size == itw.chain_bytes("bc1a", sizes)
    levels = itw.decode_chain("bc1a", blocks, sizes)
    for l, (lv, row) in enumerate(zip(levels, rows)):
        assert int(row.texels) == sizes[l][0] * sizes[l][1]
        assert int((lv[..., 3] == 255).sum()) == int(row.covered), (l, sizes[l], int((lv[..., 3] == 255).sum()), int(row.covered))
        assert set(np.unique(lv[..., 3])) <= {0, 255}
    # the payload is the chain encoder's over the same generated chain
    chain, _ = itw.generate_mips(base, alpha_coverage=r, report=True)
    ok2, again = itw.compress_chain("bc1a", chain, settings=s)
    assert ok2 and np.array_equal(again, blocks)
    want = np.concatenate([want_stream(("mip", h, w, r, l), np.ascontiguousarray(lv), itw.Bc1aSettings.ref_of(r), 0) for l, lv in enumerate(chain)])
    assert np.array_equal(blocks, want)
