"""itwDecodeChain / itwDecodeImage (include/itw_decode.h): every image of a chain in one launch, any size, cropped stores.

Every comparison is ==.  The expected texels are the oracle's from-spec decode (pinned to DirectXTex's on every mode and partition by
tests/test_block_sweep.py) at the padded size 4*ceil(w/4) x 4*ceil(h/4), cropped with numpy; for the SNORM pair the integer rule of
include/itw_decode.h as tests/_dxtex_snorm.py states it.  Shapes are the smallest at which the launch shape can go wrong."""
import ctypes as C

import numpy as np
import pytest

import _dxtex_snorm
from _guarded import guarded, pattern

pytestmark = pytest.mark.gpu

FORMATS = ["bc1", "bc3", "bc4", "bc5", "bc4_snorm", "bc5_snorm", "bc7", "bc6h"]
FILL_ALPHA = {"bc4": 255, "bc5": 255, "bc4_snorm": 127, "bc5_snorm": 127, "bc6h": 0x3C00}
CROSS = [(2, 1), (0, 1), (1, 0), (1, 2), (1, 1), (3, 1)]           # (column, row) of face i: the reference's crossedCoords
_cache = {}


def _chain_sizes(w, h):
    """(h, w) of a full 2D mip chain."""
    out = [(h, w)]
    while w > 1 or h > 1:
        w, h = max(1, w >> 1), max(1, h >> 1)
        out.append((h, w))
    return out


def _nblocks(sizes):
    return [((w + 3) // 4) * ((h + 3) // 4) for h, w in sizes]


def _random_blocks(itw, fmt, nb, seed):
    rng = np.random.default_rng(seed)
    bpb = itw.BYTES_PER_BLOCK[fmt]
    b = rng.integers(0, 256, size=(nb, bpb), dtype=np.uint8)
    if fmt == "bc7":                                             # the unary mode prefix spread evenly, reserved blocks included
        for i in range(nb):
            m = i % 9
            b[i, 0] = (int(b[i, 0]) & (0xff & ~((1 << min(m + 1, 8)) - 1))) | ((1 << m) & 0xff)
    if fmt in ("bc4_snorm", "bc5_snorm"):                        # endpoint bytes of -128
        b[0::5, 0] = 0x80
        b[1::7, 1] = 0x80
        if bpb == 16:
            b[2::3, 8] = 0x80
    return b.reshape(-1)


def _want_image(oracle, fmt, blocks, h, w):
    """(texels (h, w, 4), modes) of one image's blocks."""
    if fmt in ("bc4_snorm", "bc5_snorm"):
        return _dxtex_snorm.decode_int8(1 if fmt == "bc4_snorm" else 2, blocks, w, h), np.zeros(blocks.size // (8 if fmt == "bc4_snorm" else 16), np.int32)
    H, W = (h + 3) // 4 * 4, (w + 3) // 4 * 4
    dec, modes = oracle.decode(fmt, blocks, W, H)
    if fmt == "bc6h":
        full = np.empty((H, W, 4), dtype=np.uint16)
        full[..., :3] = dec
        full[..., 3] = 0x3C00
        dec = full
    assert (modes >= -1).all()
    return np.ascontiguousarray(dec[:h, :w]), modes


def _case(itw, oracle, fmt, sizes, seed=0, blocks=None):
    """A stream for `sizes` with its expected decode, computed once: (blocks, [texels], modes of the whole stream)."""
    key = (fmt, tuple(sizes), seed) if blocks is None else None
    if key is not None and key in _cache:
        return _cache[key]
    nbs = _nblocks(sizes)
    bpb = itw.BYTES_PER_BLOCK[fmt]
    if blocks is None:
        blocks = _random_blocks(itw, fmt, sum(nbs), 1000 * seed + sum(nbs) + len(fmt))
    want, modes, at = [], [], 0
    for (h, w), nb in zip(sizes, nbs):
        t, m = _want_image(oracle, fmt, blocks[at * bpb:(at + nb) * bpb], h, w)
        t.setflags(write=False)
        want.append(t)
        modes.append(m)
        at += nb
    res = (blocks, want, np.concatenate(modes))
    for a in (res[0], res[2]):
        a.setflags(write=False)
    if key is not None:
        _cache[key] = res
    return res


def _np(t, like):
    """A decoded array / tensor as numpy of the expected dtype."""
    a = t.cpu().numpy() if hasattr(t, "data_ptr") else t
    return a.view(like.dtype)


def _check_chain(itw, gpu, oracle, fmt, sizes, device, seed=0):
    import torch
    blocks, want, want_modes = _case(itw, oracle, fmt, sizes, seed)
    src = torch.from_numpy(np.array(blocks)).to(gpu) if device else blocks
    texels, modes, amin = itw.decode_chain(fmt, src, list(sizes), want_modes=True, want_min_alpha=True)
    if device:
        torch.cuda.synchronize()
    assert len(texels) == len(sizes)
    for i, (t, w) in enumerate(zip(texels, want)):
        got = _np(t, w)
        assert got.shape == w.shape and np.array_equal(got, w), (fmt, i, sizes[i], np.argwhere(got != w)[:4].tolist())
    assert np.array_equal(_np(modes, want_modes), want_modes)
    got_min = [int(v) & 0xFFFFFFFF for v in (amin.cpu().tolist() if device else amin.tolist())]
    assert got_min == [int(w[..., 3].view(np.uint8 if w.dtype == np.int8 else w.dtype).min()) for w in want], fmt


# ---- 1. every format, a full chain ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [False, True], ids=["numpy", "cuda"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_decodes_a_full_chain(itw, gpu, oracle, fmt, device):
    """37x21 -> 18x10 -> 9x5 -> 4x2 -> 2x1 -> 1x1: widths and heights of every residue mod 4, a 1-texel-wide image, four whole images in one wave."""
    sizes = _chain_sizes(37, 21)
    assert sizes == [(21, 37), (10, 18), (5, 9), (2, 4), (1, 2), (1, 1)]
    _check_chain(itw, gpu, oracle, fmt, sizes, device)
    if fmt == "bc7":
        assert set(range(-1, 8)) <= set(_case(itw, oracle, fmt, sizes)[2].tolist())


# ---- 2. boundaries of the launch shape -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["bc1", "bc7"])
def test_a_row_of_exactly_one_workgroup(itw, gpu, oracle, fmt):
    """1023 x 517: 256 x 130 blocks, a partial last column and a partial last row."""
    import torch
    blocks, want, want_modes = _case(itw, oracle, fmt, [(517, 1023)])
    got, modes = itw.decode_image(fmt, torch.from_numpy(np.array(blocks)).to(gpu), (517, 1023), want_modes=True)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want[0]) and np.array_equal(modes.cpu().numpy(), want_modes)


@pytest.mark.parametrize("fmt", ["bc3", "bc6h"])
def test_a_block_count_that_is_no_multiple_of_256(itw, gpu, oracle, fmt):
    sizes = _chain_sizes(70, 45)
    assert sum(_nblocks(sizes)) == 292                          # one full workgroup and a part of the next
    _check_chain(itw, gpu, oracle, fmt, sizes, True)


@pytest.mark.parametrize("fmt", ["bc1", "bc7"])
def test_more_images_than_lanes_in_a_wave(itw, gpu, oracle, fmt):
    """70 images of 1x1: lane j's image is found by the search, not by arithmetic."""
    _check_chain(itw, gpu, oracle, fmt, [(1, 1)] * 70, True)
    _check_chain(itw, gpu, oracle, fmt, [(1, 1)] * 70, False)


# ---- 3. extent -----------------------------------------------------------------------------------------------------------------

def _extent(itw, gpu, oracle, fmt, device, misaligned):
    import torch
    sizes = _chain_sizes(37, 21)
    blocks, want, want_modes = _case(itw, oracle, fmt, sizes)
    px = 8 if fmt == "bc6h" else 4
    shift = (px if misaligned else 0)                            # 4 (8 for bc6h) bytes past a multiple of 16
    place, at = [], 64                                           # the first image is a view at a non-zero offset of the payload
    for h, w in sizes:
        if misaligned:                                           # a stride that is a multiple of 4 (8 for bc6h) and not of 16
            stride = w * px + (36 if px == 4 else 40)
            stride += px if stride % 16 == 0 else 0
            assert stride % 16 and stride % px == 0
        else:                                                    # every row starts 16-byte aligned
            stride = (w * px + 15) // 16 * 16 + 48
        place.append((at, stride))
        at += h * stride + 64
    dev = gpu if device else None
    out = guarded(at, device=dev, offset=shift)
    modes = guarded(want_modes.size * 4, device=dev, offset=4)
    amin = guarded(len(sizes) * 4, device=dev, offset=4)
    src = torch.from_numpy(np.array(blocks)).to(gpu) if device else blocks
    surfs = (itw.RgbaSurface * len(sizes))(*[itw.RgbaSurface(out.ptr + o, w, h, s) for (h, w), (o, s) in zip(sizes, place)])
    expect = pattern(at, start=out.start)
    for (h, w), (o, s), t in zip(sizes, place, want):
        for y in range(h):
            expect[o + y * s:o + y * s + w * px] = t[y].view(np.uint8).reshape(-1)
    want_min = [int(t[..., 3].view(np.uint8 if t.dtype == np.int8 else t.dtype).min()) for t in want]
    itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
    for call in (1, 2):                                          # two consecutive calls, nothing refilled in between
        rc = itw.lib().itwDecodeChain(itw.DXGI_FORMAT[fmt], src.data_ptr() if device else src.ctypes.data, C.cast(surfs, C.c_void_p), len(sizes),
                                      modes.ptr, amin.ptr)
        assert rc == 0
        torch.cuda.synchronize()
        got = out.host()
        bad = np.flatnonzero(got != expect)
        assert bad.size == 0, (fmt, call, "payload", bad[:8].tolist(), place)
        for g, name in ((out, "texels"), (modes, "modes"), (amin, "min_alpha")):
            g.check(f"decode chain {fmt} call {call}: {name}")
        assert np.array_equal(modes.host().view(np.int32), want_modes)
        assert amin.host().view(np.uint32).tolist() == want_min


@pytest.mark.parametrize("misaligned", [False, True], ids=["vector-rows", "dword-rows"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_only_the_texels_of_each_image_are_written_device(itw, gpu, oracle, fmt, misaligned):
    _extent(itw, gpu, oracle, fmt, True, misaligned)


@pytest.mark.parametrize("misaligned", [False, True], ids=["vector-rows", "dword-rows"])
@pytest.mark.parametrize("fmt", ["bc1", "bc5_snorm", "bc7", "bc6h"])
def test_only_the_texels_of_each_image_are_written_host(itw, gpu, oracle, fmt, misaligned):
    _extent(itw, gpu, oracle, fmt, False, misaligned)


# ---- 4. cross layout -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["bc7", "bc6h"])
def test_six_faces_decode_straight_into_a_horizontal_cross(itw, gpu, oracle, fmt):
    """Six 20x20 faces (5x5 blocks: whole blocks, rows that are no whole waves) into an 80x60 canvas: ConvertToHorizontalCrossFromCubeMap with no copy."""
    import torch
    s = 20
    blocks, want, _ = _case(itw, oracle, fmt, [(s, s)] * 6, seed=4)
    px = 8 if fmt == "bc6h" else 4
    g = guarded(3 * s * 4 * s * px, device=gpu)
    canvas = g.view.view(torch.int16 if fmt == "bc6h" else torch.uint8).view(3 * s, 4 * s, 4)
    outs = [canvas[r * s:(r + 1) * s, c * s:(c + 1) * s] for c, r in CROSS]
    itw.decode_chain(fmt, torch.from_numpy(np.array(blocks)).to(gpu), outs)
    torch.cuda.synchronize()
    g.check(f"cross {fmt}")
    got = g.host().view(want[0].dtype).reshape(3 * s, 4 * s, 4)
    empty = pattern(g.nbytes, start=g.start).view(want[0].dtype).reshape(3 * s, 4 * s, 4)
    for r in range(3):
        for c in range(4):
            cell = got[r * s:(r + 1) * s, c * s:(c + 1) * s]
            if (c, r) in CROSS:
                assert np.array_equal(cell, want[CROSS.index((c, r))]), (fmt, c, r)
            else:
                assert np.array_equal(cell, empty[r * s:(r + 1) * s, c * s:(c + 1) * s]), (fmt, "empty cell", c, r)


# ---- 5. min_alpha --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["bc1", "bc3", "bc7"])
def test_min_alpha_is_the_minimum_over_the_stored_texels(itw, gpu, oracle, fmt):
    """(_check_chain compares min_alpha with the numpy minimum of the cropped oracle alpha.)  The random streams give images with and without
    transparent texels; bc1's have punch-through blocks."""
    sizes = _chain_sizes(37, 21) + [(3, 3), (1, 5), (8, 8)]
    _, want, _ = _case(itw, oracle, fmt, sizes, seed=5)
    mins = [int(w[..., 3].min()) for w in want]
    assert len(set(mins)) > 1, mins                              # the case distinguishes images
    if fmt == "bc1":
        assert 0 in mins and 255 in mins
    _check_chain(itw, gpu, oracle, fmt, sizes, True, seed=5)
    _check_chain(itw, gpu, oracle, fmt, sizes, False, seed=5)


def test_a_transparent_texel_in_the_padding_does_not_count(itw, gpu, oracle):
    """bc1, 5x5 (2x2 blocks): the only punch-through texel is texel (5, 0), in the padding of the right edge block: the image reports 255."""
    import torch
    opaque = np.frombuffer(np.array([0xFFFF, 0x0000], np.uint16).tobytes() + np.array([0x1B1B1B1B], np.uint32).tobytes(), np.uint8)     # c0 > c1: four colours
    edge = np.frombuffer(np.array([0x0000, 0xFFFF], np.uint16).tobytes() + np.array([0x0000000C], np.uint32).tobytes(), np.uint8)       # c0 <= c1, texel 1 = index 3
    blocks = np.concatenate([opaque, edge, opaque, opaque, opaque, edge, opaque, opaque])      # image 0: 5x5; image 1: 6x5 shows the texel
    sizes = [(5, 5), (5, 6)]
    _, want, _ = _case(itw, oracle, "bc1", sizes, blocks=blocks)
    padded, _ = oracle.decode("bc1", blocks[:32], 8, 8)
    assert int(padded[..., 3].min()) == 0 and int(padded[0, 5, 3]) == 0 and int(want[0][..., 3].min()) == 255 and int(want[1][..., 3].min()) == 0
    for src in (blocks, torch.from_numpy(blocks.copy()).to(gpu)):
        texels, amin = itw.decode_chain("bc1", src, sizes, want_min_alpha=True)
        assert [int(v) for v in (amin.cpu().tolist() if hasattr(amin, "cpu") else amin.tolist())] == [255, 0]
        assert all(np.array_equal(_np(t, w), w) for t, w in zip(texels, want))
        one = itw.decode_image("bc1", src[:32], (5, 5), want_min_alpha=True)[1]
        assert int(one if isinstance(one, int) else one.item()) == 255


@pytest.mark.parametrize("fmt", sorted(FILL_ALPHA))
def test_the_fill_formats_report_their_constant(itw, gpu, oracle, fmt):
    import torch
    sizes = [(5, 9), (1, 1)]
    blocks, _, _ = _case(itw, oracle, fmt, sizes)
    _, amin = itw.decode_chain(fmt, torch.from_numpy(np.array(blocks)).to(gpu), sizes, want_min_alpha=True)
    assert amin.cpu().tolist() == [FILL_ALPHA[fmt]] * 2


# ---- 6. agreement with what exists ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_image_writes_what_decode_blocks_writes(itw, gpu, oracle, fmt):
    import torch
    rng_blocks = _random_blocks(itw, fmt, 32 * 16, 77)
    d = torch.from_numpy(rng_blocks).to(gpu)
    a, am = itw.decode(fmt, d, 128, 64, want_modes=True)
    b, bm = itw.decode_image(fmt, d, (64, 128), want_modes=True)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(am, bm)
    h, hm = itw.decode_image(fmt, rng_blocks, (64, 128), want_modes=True)      # and through host pointers
    assert np.array_equal(h, a.cpu().numpy()) and np.array_equal(hm, am.cpu().numpy())


@pytest.mark.parametrize("fmt,profile", [("bc7", "veryfast"), ("bc1", None), ("bc5_snorm", None)])
def test_the_three_chain_calls_describe_one_stream(itw, gpu, fmt, profile):
    """compress_chain -> decode_chain -> numpy sums == measure_chain, per image and channel, as integers."""
    import torch
    from itw_amd import surfaces
    top = surfaces.snorm_normal_map(600, 1000) if fmt == "bc5_snorm" else surfaces.ldr_smooth(600, 1000)
    assert top.shape == (600, 1000, 4)
    levels = [torch.from_numpy(np.ascontiguousarray(top[:h, :w])).to(gpu) for h, w in _chain_sizes(1000, 600)]      # crops: any content will do
    ok, blocks = itw.compress_chain(fmt, levels, profile=profile)
    assert ok
    decoded = itw.decode_chain(fmt, blocks, [tuple(lv.shape[:2]) for lv in levels])
    stats = itw.measure_chain(fmt, blocks, levels)
    torch.cuda.synchronize()
    for i, (lv, dec, st) in enumerate(zip(levels, decoded, stats)):
        s = lv.cpu().numpy().astype(np.int64)
        if fmt == "bc5_snorm":
            s[s == -128] = -127                                  # both mean -1.0 (include/itw_decode.h)
        diff = s - dec.cpu().numpy().astype(np.int64)
        assert (st.width, st.height) == (lv.shape[1], lv.shape[0])
        assert [int(v) for v in st.sse] == [int((diff[..., c] ** 2).sum()) for c in range(4)], (fmt, i)
        assert [int(v) for v in st.max_abs] == [int(np.abs(diff[..., c]).max()) for c in range(4)], (fmt, i)


# ---- 7. DDS --------------------------------------------------------------------------------------------------------------------

def test_a_mipped_cube_loads_from_dds(itw, gpu, oracle):
    sizes = _chain_sizes(16, 16) * 6
    assert len(sizes) == 30
    blocks, want, _ = _case(itw, oracle, "bc3", sizes, seed=7)
    nbs = _nblocks(sizes)
    offs = np.concatenate([[0], np.cumsum(nbs)]) * 16
    data = itw.dds_file("bc3", 16, 16, [blocks[offs[i]:offs[i + 1]] for i in range(30)], mip_levels=5, cubemap=True)
    want_min = [int(w[..., 3].min()) for w in want]
    for device in (None, gpu):
        desc, texels, amin = itw.load_dds(data.tobytes() if device is None else data, device=device)
        assert (desc.width, desc.height, desc.mip_levels, desc.dxgi_format, desc.is_cubemap, desc.array_size) == (16, 16, 5, 77, 1, 1)
        assert [tuple(t.shape) for t in texels] == [(h, w, 4) for h, w in sizes]
        assert all(np.array_equal(_np(t, w), w) for t, w in zip(texels, want))
        assert amin == want_min
    for cut in (data[:-1], data[:128], data[:100]):
        with pytest.raises(ValueError):
            itw.load_dds(cut)


def test_mixed_host_and_device_outputs_are_refused(itw, gpu):
    import torch
    host = np.zeros((4, 4, 4), np.uint8)
    dev = torch.zeros((4, 4, 4), dtype=torch.uint8, device=gpu)
    blocks = np.zeros(32, np.uint8)
    for outs in ([host, dev], [dev, host]):
        surfs = (itw.RgbaSurface * 2)(*[itw.RgbaSurface(o.data_ptr() if hasattr(o, "data_ptr") else o.ctypes.data, 4, 4, 16) for o in outs])
        assert itw.lib().itwDecodeChain(71, blocks.ctypes.data, C.cast(surfs, C.c_void_p), 2, None, None) == -1
    torch.cuda.synchronize()
    assert int(dev.sum().item()) == 0 and int(host.sum()) == 0
