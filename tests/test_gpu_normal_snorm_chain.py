"""itwCompressSignedNormalMapChain (include/itw_dispatch.h): a chain of signed normal sources to BC4_SNORM / BC5_SNORM in one call.  The stream
is byte for byte the chain call (itwCompressImageChainEx) over images quantised by the numpy model (tests/_normal_snorm.py); the sources are
not written and nothing is written outside the stream.  On the parent commit the symbol does not exist: every case here fails there."""
import numpy as np
import pytest

import _guarded as G
import _normal_snorm as S

KINDS, content, _torch_of = S.KINDS, S.content, S.torch_of

pytestmark = pytest.mark.gpu
FORMATS = ("bc4_snorm", "bc5_snorm")      # DXGI 81, 84
_want = {}


def chain_sizes(name):
    """(width, height) of every image: a 37 x 21 2D chain down to 1 x 1, or the six faces of a 16^2 cube with their mips, face after face"""
    if name == "2d":
        return [(37, 21), (18, 10), (9, 5), (4, 2), (2, 1), (1, 1)]
    return [(16 >> l, 16 >> l) for _ in range(6) for l in range(5)]


def sources(kind, name):
    return [content(kind, h, w, 1000 * i + 7 * w + h) for i, (w, h) in enumerate(chain_sizes(name))]


def wanted(itw, gpu, fmt, kind, name, ops):
    """the chain call over the model's images, computed once per case"""
    key = (fmt, kind, name, ops)
    if key not in _want:
        import torch
        q = [torch.from_numpy(np.ascontiguousarray(S.quantize(s, ops))).to(gpu) for s in sources(kind, name)]
        ok, out = itw.compress_chain(fmt, q)
        assert ok
        _want[key] = out.cpu().numpy()
    return _want[key]


def _as_arrays(kind, srcs):
    return [s.view(np.int16) if s.dtype == np.uint16 else s for s in srcs]


@pytest.mark.parametrize("layout", ["as they lie", "strided views"])
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("name", ["2d", "cube"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_chain_stream_is_the_chain_call_over_quantised_images(itw, gpu, fmt, kind, name, where, layout):
    import torch
    ops = 7
    srcs = _as_arrays(kind, sources(kind, name))
    want = wanted(itw, gpu, fmt, kind, name, ops)
    dev = gpu if where == "device" else None
    pad = 0 if layout == "as they lie" else 3 * S.texel_bytes(srcs[0])
    frozen = [G.frozen(s, row_pad=pad, device=dev) for s in srcs]
    out = G.guarded(want.size, device=dev)
    ok, _ = itw.compress_chain_normal_snorm(fmt, [f.view for f in frozen], ops=ops, out=out.view)
    if dev is not None:
        torch.cuda.synchronize()
    assert ok and itw.last_error() is None
    out.check("the stream's guards")
    for f in frozen:
        f.check("a source")
    bpb = 8 if fmt == "bc4_snorm" else 16
    got = out.host()
    bad = np.nonzero((got.reshape(-1, bpb) != want.reshape(-1, bpb)).any(axis=1))[0]
    assert bad.size == 0, (bad.size, int(bad[0]))


@pytest.mark.parametrize("ops", [0, 3, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_the_other_ops_on_the_2d_chain(itw, gpu, kind, ops):
    srcs = [_torch_of(s, gpu) for s in sources(kind, "2d")]
    ok, got = itw.compress_chain_normal_snorm("bc5_snorm", srcs, ops=ops)
    assert ok and np.array_equal(got.cpu().numpy(), wanted(itw, gpu, "bc5_snorm", kind, "2d", ops))


@pytest.mark.parametrize("where", ["device", "host"])
def test_progress_is_called_for_every_image_in_order_and_stops_the_job(itw, gpu, where):
    srcs = _as_arrays("half", sources("half", "cube"))
    n = len(srcs)
    want = wanted(itw, gpu, "bc5_snorm", "half", "cube", 7)
    ends = np.cumsum([((h + 3) // 4) * ((w + 3) // 4) * 16 for w, h in chain_sizes("cube")])
    src = srcs if where == "host" else [_torch_of(s, gpu) for s in srcs]
    calls = []
    ok, got = itw.compress_chain_normal_snorm("bc5_snorm", src, ops=7, progress=lambda i, t, u: calls.append((i, t)) or True)
    assert ok and calls == [(i, n) for i in range(1, n + 1)]
    k = 4
    calls = []

    def prog(i, t, u):
        calls.append(i)
        return i != k

    ok, got = itw.compress_chain_normal_snorm("bc5_snorm", src, ops=7, progress=prog)
    assert ok is False and calls == list(range(1, k + 1)), calls
    written = int(ends[k - 2])
    got = got.cpu().numpy() if where == "device" else got
    assert np.array_equal(got[:written], want[:written])


def test_a_large_level_goes_through_the_gather_too(itw, gpu):
    """an image of a window's worth of blocks and whole-block size would be encoded in place by the chain call; a signed source never is"""
    import torch
    rng = np.random.default_rng(5)
    base = rng.normal(0, 0.5, (2048, 2048, 4)).astype(np.float32)
    srcs = [base, np.ascontiguousarray(base[::2, ::2]), np.ascontiguousarray(base[:5, :7])]
    q = [torch.from_numpy(np.ascontiguousarray(S.quantize(s, 7))).to(gpu) for s in srcs]
    ok, want = itw.compress_chain("bc5_snorm", q)
    assert ok
    ok, got = itw.compress_chain_normal_snorm("bc5_snorm", [torch.from_numpy(s).to(gpu) for s in srcs], ops=7)
    assert ok and torch.equal(got, want)


# ---- the mipped call ------------------------------------------------------------------------------------------------------------------------

def widen_model(base, ops):
    """level 0 of the mipped call as RGBA16F bits: int8 -> half(load rule), half copied, float by the mip filter's store rule; the flips are the
    sign bits of x and y"""
    if base.dtype == np.int8:
        bits = S.load(base).astype(np.float16).view(np.uint16).copy()
    elif base.dtype.itemsize == 2:
        bits = base.view(np.uint16).copy()
    else:
        with np.errstate(invalid="ignore"):
            bits = np.clip(base, np.float32(-65504.0), np.float32(65504.0)).astype(np.float16).view(np.uint16).copy()
        bits[np.isnan(base)] = 0x7E00
    if ops & 1:
        bits[..., 0] ^= 0x8000
    if ops & 2:
        bits[..., 1] ^= 0x8000
    return bits


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("items", [1, 6])
@pytest.mark.parametrize("size", [(64, 64), (100, 36)], ids=["64x64-pyramid", "100x36-linear"])
@pytest.mark.parametrize("kind", KINDS)
def test_mipped_call_is_the_composition_of_the_public_stages(itw, gpu, kind, size, items, where):
    import torch
    w, h = size
    ops = 7
    bases = _as_arrays(kind, [content(kind, h, w, 50 + i) for i in range(items)])
    # the composition written out: the model's widening, itwGenerateMipChain, the chain call with the normalise alone
    chains = itw.generate_mips([_torch_of(widen_model(b, ops), gpu) for b in bases])
    ok, want = itw.compress_chain_normal_snorm("bc5_snorm", [lv for ch in chains for lv in ch], ops=ops & 4)
    assert ok
    dev = gpu if where == "device" else None
    frozen = [G.frozen(b, device=dev) for b in bases]
    out = G.guarded(want.numel(), device=dev)
    ok, _ = itw.compress_mipped_normal_snorm("bc5_snorm", [f.view for f in frozen], ops=ops, out=out.view)
    if dev is not None:
        torch.cuda.synchronize()
    assert ok and itw.last_error() is None
    out.check("the stream's guards")
    for f in frozen:
        f.check("a base")
    assert np.array_equal(out.host(), want.cpu().numpy())


def test_int8_minus_one_and_plus_one_average_to_zero(itw, gpu):
    """the case the biased RGBA8 filter gets wrong (0xFF and 0x01 average to 0x80 = -128): the signed path's level 1 is code 0"""
    base = np.zeros((2, 2, 4), np.int8)
    base[..., 0] = [[-1, 1], [1, -1]]
    base[..., 1] = [[1, -1], [-1, 1]]
    ok, got = itw.compress_mipped_normal_snorm("bc5_snorm", base)
    ok2, want = itw.compress_chain("bc5_snorm", [base, np.zeros((1, 1, 4), np.int8)])
    assert ok and ok2 and np.array_equal(got, want)
    ok3, biased = itw.compress_chain("bc5_snorm", [base, np.full((1, 1, 4), -128, np.int8)])
    assert ok3 and not np.array_equal(got, biased)
