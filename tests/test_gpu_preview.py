"""itwPreviewBlocks / itwPreviewSurface (include/itw_decode.h): a viewport of an image, decoded where it is looked at.

Every comparison is == against tests/_preview.py (pinned to literals from the reference's text by tests/test_preview_cpu.py), applied to the
oracle's from-spec decode exactly as tests/test_gpu_decode_chain.py obtains it.  Shapes are the smallest at which the launch can go wrong:
images of every residue mod 4, viewports that are a multiple of no tile shape, zooms on both sides of the route switch."""
import ctypes as C

import numpy as np
import pytest

import _etc1
import _preview
from _guarded import guarded, rows_of
from test_gpu_decode_chain import _random_blocks, _want_image

pytestmark = pytest.mark.gpu

FORMATS = ["bc1", "bc3", "bc4", "bc5", "bc7", "bc6h", "etc1"]
MATTE = 0x00C86432                                               # bytes 0x32, 0x64, 0xC8: no byte equals another
_cache = {}


def _image(itw, oracle, fmt, w, h, seed=0):
    """(blocks, texels (h, w, 4)) of a random stream, computed once and left unchanged."""
    key = (fmt, w, h, seed)
    if key not in _cache:
        nb = ((w + 3) // 4) * ((h + 3) // 4)
        blocks = _random_blocks(itw, fmt, nb, 7000 + 13 * seed + nb + len(fmt))
        if fmt == "etc1":
            texels = np.ascontiguousarray(_etc1.decode_np(blocks, (w + 3) // 4 * 4, (h + 3) // 4 * 4)[0][:h, :w])
        else:
            texels, modes = _want_image(oracle, fmt, blocks, h, w)
            if fmt == "bc7":
                assert set(range(-1, 8)) <= set(modes.tolist())  # every mode and the reserved prefix
        for a in (blocks, texels):
            a.setflags(write=False)
        _cache[key] = (blocks, texels)
    return _cache[key]


def _show(itw, gpu, fmt, blocks, w, h, device, **view):
    """itw.preview through host or device pointers, as numpy."""
    import torch
    if not device:
        return itw.preview(fmt, blocks, w, h, **view)
    got = itw.preview(fmt, torch.from_numpy(np.array(blocks)).to(gpu), w, h, **view)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _want(texels, view_w, view_h, x=0, y=0, zoom=1.0, channels="rgb", matte=0, exposure=1.0):
    options = channels if isinstance(channels, int) else sum({{"r": 4, "g": 8, "b": 16, "a": 32}[c] for c in channels})
    return _preview.viewport(texels, view_w, view_h, x, y, zoom, options, matte, exposure)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, (what, len(bad), [(int(r), int(c), got[r, c].tolist(), want[r, c].tolist()) for r, c in bad[:4]])


# ---- 1. every format, one full view --------------------------------------------------------------------------------------------------

FULL_VIEW = dict(view_w=50, view_h=30, x=-5, y=-3, zoom=1.0, matte=MATTE)


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "cuda"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_shows_every_texel_once(itw, gpu, oracle, fmt, device):
    """37 x 21 under a 50 x 30 view at (-5, -3), zoom 1: matte on all four sides, every texel once, the padding of the edge blocks never."""
    blocks, texels = _image(itw, oracle, fmt, 37, 21)
    want = _want(texels, **FULL_VIEW)
    matte = np.array([0x32, 0x64, 0xC8], np.uint8)
    assert (want[:3] == matte).all() and (want[24:] == matte).all() and (want[:, :5] == matte).all() and (want[:, 42:] == matte).all()
    if fmt != "bc6h":
        assert np.array_equal(want[3:24, 5:42], texels[..., :3])
    _same(_show(itw, gpu, fmt, blocks, 37, 21, device, **FULL_VIEW), want, (fmt, device))


# ---- 2. zoom sweep across the route switch -------------------------------------------------------------------------------------------

def _zooms(itw):
    t = itw.PREVIEW_TILE_MAX_ZOOM
    return [1 / 8, float(np.float32(1 / 3)), 0.5, 1.0, 1.5, 2.0, float(np.nextafter(t, 0.0)), t, float(np.nextafter(t, 4.0)), 4.0, 16.0, 1000.0]


@pytest.mark.parametrize("fmt", ["bc7", "bc6h"])
def test_zoom_sweep_across_the_route_switch(itw, gpu, oracle, fmt):
    """131 x 67 under a 97 x 41 viewport (a multiple of no tile shape, two tiles across and three down) at every zoom, from offsets that put
    the view before the image, at its origin, inside it and across its far edge."""
    import torch
    w, h = 131, 67
    blocks, texels = _image(itw, oracle, fmt, w, h)
    d = torch.from_numpy(np.array(blocks)).to(gpu)
    zooms = _zooms(itw)
    assert zooms[6] < zooms[7] == 2.0 < zooms[8] and len(set(zooms)) == 11
    for zoom in zooms:
        inside = (int(40 / zoom), int(20 / zoom))
        far = (int(w / zoom) - 60, int(h / zoom) - 25)
        for x, y in ((-7, -5), (0, 0), inside, far):
            view = dict(view_w=97, view_h=41, x=x, y=y, zoom=zoom, matte=MATTE, exposure=0.75)
            want = _want(texels, **view)
            got = itw.preview(fmt, d, w, h, **view)
            torch.cuda.synchronize()
            _same(got.cpu().numpy(), want, (fmt, zoom, x, y))
        _same(itw.preview(fmt, blocks, w, h, **view), want, (fmt, zoom, "host"))      # the last view through host pointers: part of the stream uploaded
    shown = _want(texels, 97, 41, far[0], far[1], 1000.0, matte=MATTE)
    assert (shown != np.array([0x32, 0x64, 0xC8], np.uint8)).any()                       # zoom 1000 still shows texels here


# ---- 3. the fraction rule ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [False, True], ids=["numpy", "cuda"])
def test_the_fraction_rule(itw, gpu, oracle, device):
    """zoom 0.5: xt + x_offset = -1 gives fx = -0.5 and shows column 0; -2 gives -1.0 and shows the matte.  Rows likewise."""
    blocks, texels = _image(itw, oracle, "bc3", 37, 21)
    got = _show(itw, gpu, "bc3", blocks, 37, 21, device, view_w=20, view_h=12, x=-3, y=-4, zoom=0.5, matte=MATTE)
    matte = [0x32, 0x64, 0xC8]
    assert got[3, 1].tolist() == matte and got[2, 2].tolist() == matte              # xt + xo = -2; yt + yo = -2
    assert got[3, 2].tolist() == texels[0, 0, :3].tolist()                          # (-1, -1) -> texel (0, 0)
    assert got[4, 2].tolist() == texels[0, 0, :3].tolist() and got[5, 3].tolist() == texels[0, 0, :3].tolist()      # (-1, 0), (0, 1) too
    assert got[6, 5].tolist() == texels[1, 1, :3].tolist()
    _same(got, _want(texels, 20, 12, -3, -4, 0.5, matte=MATTE), device)
    far = _show(itw, gpu, "bc3", blocks, 37, 21, device, view_w=70, view_h=20, x=2 ** 30, y=0, zoom=1000.0, matte=MATTE)
    assert (far == np.array(matte, np.uint8)).all()                                 # 2^30 * 1000 is beyond the int range: outside
    far = _show(itw, gpu, "bc3", blocks, 37, 21, device, view_w=70, view_h=20, x=-2 ** 30, y=-2 ** 30, zoom=1.75, matte=MATTE)
    assert (far == np.array(matte, np.uint8)).all()


# ---- 4. all 16 channel masks ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,exposure", [("bc3", 1.0), ("bc6h", 2.0)])
def test_all_16_channel_masks(itw, gpu, oracle, fmt, exposure):
    import torch
    blocks, texels = _image(itw, oracle, fmt, 37, 21)
    d = torch.from_numpy(np.array(blocks)).to(gpu)
    if fmt == "bc3":
        assert len(np.unique(texels[..., 3])) > 16               # real alpha
    for m in range(16):
        options = (m << 2) | 0x43                                # bits outside the mask are ignored
        view = dict(FULL_VIEW, channels=options, exposure=exposure)
        got = itw.preview(fmt, d, 37, 21, **view)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        _same(got, _want(texels, **view), (fmt, hex(options)))
        if fmt == "bc6h" and m == 8:                             # alpha alone: 1.0 at exposure 1, whatever the exposure asked for
            assert (got[3:24, 5:42] == 255).all()
        if m == 12:                                              # blue and alpha: alpha, with nothing in the other two bytes
            assert (got[3:24, 5:42, :2] == 0).all()
    _same(itw.preview(fmt, blocks, 37, 21, **view), _want(texels, **view), (fmt, "host"))


# ---- 5. tone sweep, through itwPreviewSurface ----------------------------------------------------------------------------------------

def _half_surface():
    if "halves" not in _cache:
        p = np.arange(65536, dtype=np.uint32).reshape(256, 256)
        s = np.stack([p, p ^ 0x8000, ~p & 0xFFFF, (p * 40503) & 0xFFFF], axis=2).astype(np.uint16)
        s.setflags(write=False)
        _cache["halves"] = s
    return _cache["halves"]


@pytest.mark.parametrize("exposure", [1.0, 0.5, float(np.float32(2.2)), float(np.float32(1 / 3)), 255.0, 1e-3, 0.0, -1.0, float("inf")])
def test_tone_of_every_half_pattern(itw, gpu, exposure):
    """All 65 536 half patterns in R, their negations in G, their complements in B, at zoom 1: FloatToByte((float)half * exposure)."""
    import torch
    s = _half_surface()
    want = _preview.viewport(s, 256, 256, exposure=exposure)
    got = itw.preview_surface(torch.from_numpy(np.array(s).view(np.int16)).to(gpu), 256, 256, exposure=exposure)
    torch.cuda.synchronize()
    _same(got.cpu().numpy(), want, exposure)
    if exposure in (1.0, 1e-3):
        _same(itw.preview_surface(s, 256, 256, exposure=exposure), want, (exposure, "host"))
        a = itw.preview_surface(s, 256, 256, channels="ba", exposure=exposure)      # byte 2 shows alpha, with the exposure
        _same(a, _preview.viewport(s, 256, 256, options=0x30, exposure=exposure), (exposure, "ba"))


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "cuda"])
def test_an_rgba8_surface_through_the_same_views(itw, gpu, device):
    """A random 37 x 21 RGBA8 surface, rows 11 bytes apart from tight, through the full view and two zooms: the viewport arithmetic with no
    decoder taking part."""
    import torch
    rng = np.random.default_rng(37)
    full = rng.integers(0, 256, size=(21, 40, 4), dtype=np.uint8)
    img = full[:, :37]
    src = torch.from_numpy(full).to(gpu)[:, :37] if device else img
    for view in (FULL_VIEW, dict(view_w=97, view_h=41, x=-9, y=-6, zoom=0.25, matte=MATTE, channels="ga"),
                 dict(view_w=33, view_h=9, x=-2, y=-1, zoom=3.5, matte=MATTE, channels="r")):
        got = itw.preview_surface(src, **view)
        if device:
            torch.cuda.synchronize()
            got = got.cpu().numpy()
        _same(got, _want(img, **view), (device, view))


# ---- 6. write extents ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("zoom", [1.0, 4.0], ids=["tile-route", "pixel-route"])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("device", [False, True], ids=["host-out", "device-out"])
def test_only_the_rows_of_the_viewport_are_written(itw, gpu, oracle, device, offset, zoom):
    """out_rgb at base + 0 .. 3 and rows 3 * width + 5 bytes apart, so that rows start at every residue mod 4: exactly 3 * width bytes of each
    row change, whether they went out as dwords or as bytes."""
    import torch
    blocks, texels = _image(itw, oracle, "bc7", 37, 21)
    vw, vh = 50, 30
    stride = 3 * vw + 5
    g = guarded(vh * stride, device=gpu if device else None, offset=offset, rows=(vh, 3 * vw, stride))
    view = itw.preview_view(vw, vh, -5, -3, zoom, "rgb", MATTE)
    d = torch.from_numpy(np.array(blocks)).to(gpu)
    itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
    for src in (d.data_ptr(), blocks.ctypes.data):               # device and host blocks into the same kind of output
        g.refill()
        rc = itw.lib().itwPreviewBlocks(98, src, 37, 21, C.byref(view), C.sizeof(view), g.ptr, stride)
        assert rc == 0
        torch.cuda.synchronize()
        g.check(f"preview bc7 device={device} offset={offset} zoom={zoom}")
        _same(rows_of(g).reshape(vh, vw, 3), _want(texels, vw, vh, -5, -3, zoom, matte=MATTE), (device, offset, zoom))


# ---- 7. graph capture ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("zoom", [0.5, 4.0], ids=["tile-route", "pixel-route"])
def test_a_captured_preview_replays_on_changed_blocks(itw, gpu, oracle, zoom):
    """An all-device call is one launch on the caller's stream: captured once, replayed on two other streams' worth of blocks at the same
    address, each replay gives the bytes of an eager call on those blocks."""
    import torch
    w, h, vw, vh = 64, 64, 70, 40
    streams = [_image(itw, oracle, "bc7", w, h, seed=s) for s in (1, 2, 3)]
    d = torch.from_numpy(np.array(streams[0][0])).to(gpu)
    out = torch.zeros((vh, vw, 3), dtype=torch.uint8, device=gpu)
    view = itw.preview_view(vw, vh, -3, -2, zoom, "rgb", MATTE)
    L = itw.lib()
    side = torch.cuda.Stream()

    def call():
        L.itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
        assert L.itwPreviewBlocks(98, d.data_ptr(), w, h, C.byref(view), C.sizeof(view), out.data_ptr(), 3 * vw) == 0

    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        call()
    torch.cuda.synchronize()
    for blocks, texels in streams[1:]:
        d.copy_(torch.from_numpy(np.array(blocks)))
        out.fill_(0x5A)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        replayed = out.cpu().numpy()
        eager = itw.preview("bc7", d, w, h, vw, vh, -3, -2, zoom, matte=MATTE)
        torch.cuda.synchronize()
        assert np.array_equal(replayed, eager.cpu().numpy())
        _same(replayed, _want(texels, vw, vh, -3, -2, zoom, matte=MATTE), zoom)
    assert itw.last_error() is None
