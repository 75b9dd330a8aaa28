"""Height maps to normal maps on the GPU (include/itw_dispatch.h, "height maps": ITW_NORMAL_FROM_HEIGHT in the `ops` word).

itwPrepareNormalMapChain gives the reference's recorded RGBA16F bytes (tests/golden/heightmap_ref.npz) for every recorded case with a half
source, and the numpy model's bytes (tests/_height_normal.py) for RGBA8; itwQuantizeNormalMapChain gives the model's for int8, half and float
heights, and the quantised recording for the float cases.  Both run between guard bands on strided views, texel aligned and vector aligned,
over a chain of images of different sizes in one call, from host and from device pointers.  The one-call saves are compositions: their
stream is the same call without the bit over the model's (the recording's) level 0.  Device calls run in stream order with the caller's
work (the sequences of tests/_stream_order.py)."""
import ctypes as C
import json

import numpy as np
import pytest

import _guarded as G
import _height_normal as H
import _normal_snorm as S
import _stream_order as so

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 1), (1, 5), (2, 2), (7, 5), (16, 16), (65, 17), (130, 33)]        # (width, height): one chain, one call
# the fields that take another path in the kernel: channel kinds, both mirrors, invert, occlusion, and the low bits of either convention
OPS = [H.ops_word(), H.ops_word(5, True, False, True, True, 8.0, 7), H.ops_word(4, False, True, False, True, 0.5, 2), H.ops_word(2, True, True, True, False, 100.0, 5)]


@pytest.fixture(scope="module")
def recording():
    with open(H.GOLDEN_SHA) as f:
        pins = json.load(f)
    return dict(np.load(H.GOLDEN)), pins


def _with_specials(img):
    """a NaN and an Inf height among the content of a half or float image"""
    img = img.copy()
    h, w = img.shape[:2]
    if img.dtype in (np.uint16, np.float32) and w * h > 4:
        f = img.view(np.float16) if img.dtype == np.uint16 else img
        f[h // 2, w // 2] = np.nan
        f[0, 0] = np.inf
    return img


def _place(itw, gpu, where, imgs, pad, offset, frozen):
    """The images as strided regions between guard bands, on the device or the host: (regions, surface array).  frozen: sources, which a
    call must leave as they are; otherwise regions a call may write inside width x height."""
    import torch
    dev = gpu if where == "device" else None
    regions, surfs = [], []
    for a in imgs:
        h, w = a.shape[:2]
        rb = w * 4 * a.itemsize
        if frozen:
            r = G.frozen(a.view(np.int16) if a.dtype == np.uint16 else a, row_pad=pad, device=dev, offset=offset)
        else:
            r = G.guarded(h * (rb + pad), device=dev, offset=offset, rows=(h, rb, rb + pad))
            rows = np.ascontiguousarray(a).view(np.uint8).reshape(h, rb)
            if dev is None:
                r.view.reshape(h, rb + pad)[:, :rb] = rows
            else:
                r.view.view(h, rb + pad)[:, :rb].copy_(torch.from_numpy(rows))
        regions.append(r)
        surfs.append(itw.RgbaSurface(r.ptr, w, h, rb + pad))
    if dev is not None:
        torch.cuda.synchronize()
        itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
    return regions, (itw.RgbaSurface * len(surfs))(*surfs)


def _prepare(itw, gpu, where, imgs, ops, pad=0, offset=0):
    """itwPrepareNormalMapChain over copies of `imgs` in guarded regions; returns the images after the call."""
    import torch
    regions, arr = _place(itw, gpu, where, imgs, pad, offset, False)
    assert itw.lib().itwPrepareNormalMapChain(C.cast(arr, C.c_void_p), len(imgs), 4 * imgs[0].itemsize, ops) == 0, itw.last_error()
    if where == "device":
        torch.cuda.synchronize()
    out = []
    for r, a in zip(regions, imgs):
        r.check(f"image {a.shape}")
        out.append(G.rows_of(r, a.dtype).reshape(a.shape))
    return out


def _quantize(itw, gpu, where, imgs, ops, pad=0, offset=0):
    import torch
    tb = S.texel_bytes(imgs[0])
    src, sarr = _place(itw, gpu, where, imgs, pad * (tb // 4), offset * (tb // 4), True)
    dst, darr = _place(itw, gpu, where, [np.zeros(a.shape, np.int8) for a in imgs], pad, offset, False)
    assert itw.lib().itwQuantizeNormalMapChain(C.cast(sarr, C.c_void_p), tb, C.cast(darr, C.c_void_p), len(imgs), ops) == 0, itw.last_error()
    if where == "device":
        torch.cuda.synchronize()
    out = []
    for s, d, a in zip(src, dst, imgs):
        s.check(f"source {a.shape}")
        d.check(f"target {a.shape}")
        out.append(G.rows_of(d, np.int8).reshape(a.shape))
    return out


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, f"{len(bad)} components differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}")


def test_prepare_gives_every_recorded_rgba16f_byte(itw, gpu, recording):
    """every recorded case with a half source, stored whole or as a hash; under MIRROR_V row 0 is the model's (the stated divergence)"""
    import hashlib
    arrays, pins = recording
    n = 0
    for c in H.golden_cases():
        if c["src"] != "half":
            continue
        name = H.golden_name(c)
        base = H.golden_input("half", c["content"], c["height"], c["width"], c["seed"])
        got = _prepare(itw, gpu, "device", [base], c["ops"])[0]
        first = pins[name]["first_row"]
        if pins[name]["stored"]:
            _same(got[first:], arrays[name + "_f16"][first:], name)
        assert hashlib.sha256(np.ascontiguousarray(got[first:]).tobytes()).hexdigest() == pins[name]["f16_sha256"], name
        if first:
            _same(got[:1], H.to_rgba16f(base, c["ops"])[:1], name + " row 0")
        n += 1
    assert n >= 60


def test_quantize_gives_the_quantised_recording_for_float_heights(itw, gpu, recording):
    arrays, pins = recording
    n = 0
    for c in H.golden_cases():
        name = H.golden_name(c)
        if c["src"] != "float" or not pins[name]["stored"]:
            continue
        base = H.golden_input("float", c["content"], c["height"], c["width"], c["seed"])
        got = _quantize(itw, gpu, "device", [base], c["ops"])[0]
        _same(got, S.quantize_values(arrays[name + "_f32"].view(np.float32)), name)
        n += 1
    assert n >= 40


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("pad,offset", [(0, 0), (1, 1), (12, 0)], ids=["tight", "texel-aligned", "vector-aligned-rows-apart"])
@pytest.mark.parametrize("kind", ["uint8", "half"])
def test_prepare_a_chain_of_strided_views_gives_the_model_and_writes_only_its_texels(itw, gpu, kind, pad, offset, where):
    """pad and offset in texels: (1, 1) puts every row quad off the 16-byte grid (the texel-by-texel loads and stores), (12, 0) keeps it on.
    The stage itself stores a NaN as 0x7E00 (pinned by the recording above); the RGBA16F flip behind it is half(1.0f - h), and which NaN
    that gives for a NaN is not specified (include/itw_dispatch.h), so behind a flip a NaN is compared as a NaN."""
    px = 4 if kind == "uint8" else 8
    imgs = [_with_specials(H.content(kind, h, w, 40 + w)) for w, h in SIZES]

    def nan_as_one(v):
        return np.where((v & 0x7FFF) > 0x7C00, np.uint16(0x7E00), v)
    for ops in OPS:
        got = _prepare(itw, gpu, where, imgs, ops, pad * px, offset * px)
        for g, a in zip(got, imgs):
            if kind == "uint8":
                _same(g, H.to_rgba8(a, ops), (kind, a.shape, hex(ops)))
            elif ops & 3:
                _same(nan_as_one(g), nan_as_one(H.to_rgba16f(a, ops)), (kind, a.shape, hex(ops)))
            else:
                _same(g, H.to_rgba16f(a, ops), (kind, a.shape, hex(ops)))


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("pad,offset", [(0, 0), (1, 1), (12, 0)], ids=["tight", "texel-aligned", "vector-aligned-rows-apart"])
@pytest.mark.parametrize("kind", ["int8", "half", "float"])
def test_quantize_a_chain_of_strided_views_gives_the_model_and_writes_only_its_texels(itw, gpu, kind, pad, offset, where):
    imgs = [_with_specials(H.content(kind, h, w, 60 + w)) for w, h in SIZES]
    for ops in OPS:
        got = _quantize(itw, gpu, where, imgs, ops, pad * 4, offset * 4)
        for g, a in zip(got, imgs):
            _same(g, H.to_snorm(a, ops), (kind, a.shape, hex(ops)))


def test_the_binding_goes_over_both_calls(itw, gpu):
    import torch
    ops = itw.height_ops("g", "u", occlusion=True, amplitude=2.0, normalize=True)
    a = H.content("uint8", 9, 13, 5)
    t = torch.from_numpy(a).to(gpu)
    assert itw.height_to_normal(t, ops) is t
    torch.cuda.synchronize()
    _same(t.cpu().numpy(), H.to_rgba8(a, ops), "biased, device")
    b = a.copy()
    itw.height_to_normal([b], ops)
    _same(b, H.to_rgba8(a, ops), "biased, host")
    f = H.content("float", 9, 13, 6)
    out = itw.height_to_normal(torch.from_numpy(f).to(gpu), ops, kind="snorm")
    torch.cuda.synchronize()
    _same(out.cpu().numpy(), H.to_snorm(f, ops), "snorm, device")
    _same(itw.height_to_normal(f, ops, kind="snorm"), H.to_snorm(f, ops), "snorm, host")


def test_quantize_refuses_a_target_over_its_source(itw, gpu):
    """on the device too: -1 with a message, nothing written.  The error mode is process-wide: put back after the call."""
    import torch
    a = H.content("int8", 8, 8, 2)
    t = torch.from_numpy(a).to(gpu)
    s = itw.RgbaSurface(t.data_ptr(), 8, 8, 32)
    itw.set_error_mode(itw.ON_ERROR_RETURN)
    try:
        assert itw.lib().itwQuantizeNormalMapChain(C.byref(s), 4, C.byref(s), 1, H.ops_word()) == -1
        assert "overlaps" in (itw.last_error() or "")
        assert itw.lib().itwQuantizeNormalMapChain(C.byref(s), 4, C.byref(s), 1, 7) == 0           # without the bit an int8 source is its own target, as before
    finally:
        itw.lib().itwClearError()
        itw.set_error_mode(itw.ON_ERROR_ABORT)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), S.quantize(a, 7))


@pytest.mark.parametrize("w,h", [(63, 15), (64, 16), (65, 17), (128, 32), (129, 33), (200, 3), (3, 70)])
def test_single_images_around_the_tile_size(itw, gpu, w, h):
    """a workgroup takes a 64 x 16 tile: sizes below, at and above one and two tiles along either axis, the view on and off the 16-byte grid"""
    import torch
    for ops in OPS:
        for kind in ("uint8", "half"):
            a = H.content(kind, h, w, 70 + w)
            canvas = torch.zeros((h, w + 1, 4), dtype=torch.uint8 if kind == "uint8" else torch.int16, device=gpu)
            for view in (canvas[:, :w], canvas[:, 1:]):
                view.copy_(torch.from_numpy(a.view(np.int16) if kind == "half" else a))
                itw.height_to_normal(view, ops)
                torch.cuda.synchronize()
                _same(view.cpu().numpy().view(a.dtype), (H.to_rgba8 if kind == "uint8" else H.to_rgba16f)(a, ops), (kind, w, h, hex(ops)))
        for kind in ("int8", "half", "float"):
            a = H.content(kind, h, w, 80 + w)
            got = itw.height_to_normal(torch.from_numpy(a.view(np.int16) if kind == "half" else a).to(gpu), ops, kind="snorm")
            torch.cuda.synchronize()
            _same(got.cpu().numpy(), H.to_snorm(a, ops), (kind, w, h, hex(ops)))


# ---- the one-call saves: compositions ------------------------------------------------------------------------------------------------------
MIPPED = [("2d-7x5", [(7, 5)], None, ""), ("cube-16x16", [(16, 16)] * 6, None, ""), ("cubic-wrap-13x9", [(13, 9)] * 2, "cubic", "uv")]


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("fmt,profile", [("bc5", None), ("bc3", None), ("bc7", "veryfast")])
@pytest.mark.parametrize("name,sizes,filter,wrap", MIPPED, ids=[m[0] for m in MIPPED])
def test_compress_mipped_is_the_same_call_over_the_models_level_0(itw, gpu, name, sizes, filter, wrap, fmt, profile, where):
    import torch
    put = (lambda a: torch.from_numpy(a).to(gpu)) if where == "device" else (lambda a: a.copy())
    bases = [H.content("uint8", h, w, 90 + i) for i, (w, h) in enumerate(sizes)]
    for ops in OPS:
        level0 = [H.store_unorm8(H.normal(b, ops, True)) for b in bases]
        ok, got = itw.compress_mipped(fmt, [put(b) for b in bases], profile=profile, normal_ops=ops, filter=filter, wrap=wrap)
        ok2, want = itw.compress_mipped(fmt, [put(b) for b in level0], profile=profile, normal_ops=ops & 7, filter=filter, wrap=wrap)
        if where == "device":
            torch.cuda.synchronize()
            got, want = got.cpu().numpy(), want.cpu().numpy()
        assert ok and ok2 and got.size == want.size and got.size > 0
        assert np.array_equal(got, want), (name, fmt, hex(ops), int((got != want).sum()))


@pytest.mark.parametrize("where", ["device", "host"])
def test_compress_signed_mipped_is_the_same_call_over_the_recorded_rgba16f_map(itw, gpu, recording, where):
    """float and half heights; the recording's RGBA16F map with texel_bytes 8 (under MIRROR_V with a half source: the model's map)"""
    import torch
    arrays, pins = recording
    put = (lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(gpu)) if where == "device" else (lambda a: a.copy())
    n = {"half": 0, "float": 0}
    for i, c in enumerate(H.golden_cases()):
        name = H.golden_name(c)
        if not pins[name]["stored"] or c["width"] * c["height"] < 15:
            continue
        low = i % 8                                               # the flips become negations, the normalise runs in the gather
        base = H.golden_input(c["src"], c["content"], c["height"], c["width"], c["seed"])
        normals = H.store_half(H.normal(base, c["ops"], False)) if H.golden_skips_row0(c) else arrays[name + "_f16"]
        ok, got = itw.compress_mipped_normal_snorm("bc5_snorm", put(base), ops=c["ops"] | low)
        ok2, want = itw.compress_mipped_normal_snorm("bc5_snorm", put(np.ascontiguousarray(normals)), ops=low)
        if where == "device":
            torch.cuda.synchronize()
            got, want = got.cpu().numpy(), want.cpu().numpy()
        assert ok and ok2 and got.size == want.size and got.size > 0
        assert np.array_equal(got, want), (name, low, int((got != want).sum()))
        n[c["src"]] += 1
    assert n["half"] >= 15 and n["float"] >= 25


def test_compress_signed_mipped_from_int8_heights_is_the_model(itw, gpu):
    import torch
    base = H.content("int8", 12, 20, 8)
    ops = H.ops_word(3, True, False, False, True, 2.0, 6)
    ok, got = itw.compress_mipped_normal_snorm("bc4_snorm", torch.from_numpy(base).to(gpu), ops=ops)
    ok2, want = itw.compress_mipped_normal_snorm("bc4_snorm", torch.from_numpy(H.to_rgba16f_signed(base, ops & ~7).view(np.int16)).to(gpu), ops=ops & 7)
    torch.cuda.synchronize()
    assert ok and ok2 and np.array_equal(got.cpu().numpy(), want.cpu().numpy())


# ---- stream order --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env(itw, gpu, oracle):
    import torch
    delay = so.Delay(torch, gpu)
    stream = torch.cuda.Stream(gpu)
    delay(stream)
    torch.cuda.synchronize()
    e = so.Env(itw, oracle, gpu, torch, delay, stream, so.Report())
    yield e
    itw.lib().itwSetStream(None)


ORDER_SIZES = ((64, 64), (12, 20))       # (height, width)


def _prepare_case(kind):
    def build(env):
        ops = H.ops_word(5, False, True, False, True, 2.0, 3)
        contents = [[H.content(kind, h, w, 300 + 7 * k) for h, w in ORDER_SIZES] for k in range(3)]
        wants = [[np.ascontiguousarray((H.to_rgba8 if kind == "uint8" else H.to_rgba16f)(a, ops)) for a in c] for c in contents]
        return so.DeviceCase(contents, wants, [a.shape[1] * a.itemsize * 4 for a in contents[0]],
                             lambda srcs, outs: env.itw.height_to_normal(srcs, ops), in_place=True)
    return build


def _quantize_case(kind):
    def build(env):
        ops = H.ops_word(2, True, False, True, False, 8.0, 4)
        contents = [[H.content(kind, h, w, 400 + 7 * k) for h, w in ORDER_SIZES] for k in range(3)]
        wants = [[np.ascontiguousarray(H.to_snorm(a, ops)) for a in c] for c in contents]

        def call(srcs, outs):
            env.itw.height_to_normal(srcs, ops, kind="snorm", out=[o.view(env.torch.int8).view(*s.shape) for o, s in zip(outs, srcs)])
        return so.DeviceCase(contents, wants, [w * 4 for h, w in ORDER_SIZES], call)
    return build


@pytest.mark.parametrize("name,build", [("prepare-rgba8", _prepare_case("uint8")), ("prepare-rgba16f", _prepare_case("half")),
                                        ("quantize-int8", _quantize_case("int8")), ("quantize-half", _quantize_case("half")), ("quantize-float", _quantize_case("float"))],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_a_device_call_from_heights_is_in_stream_order(env, name, build):
    so.run_device("height-" + name, build(env), env, must_return_early=False)
