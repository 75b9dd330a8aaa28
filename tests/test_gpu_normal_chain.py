"""itwCompressNormalMapChain (include/itw_dispatch.h; the OPS instantiations of chain_gather_kernel, csrc/chain.hip): the stream is byte
for byte itwCompressImageChainEx over copies prepared by the numpy checker (tests/_normal_prep.py), the sources stay as they were, the
progress contract is the plain call's; and cube-cross views (itwCubeCrossFaces) feed the chain call like copied faces."""
import numpy as np
import pytest

import _normal_prep as N

pytestmark = pytest.mark.gpu


def _rgba8(h, w, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[rng.integers(0, 8, (h, w)) == 0, :3] = 128             # zero vectors: the default normal
    return img


def _rgba16f(h, w, seed):
    rng = np.random.default_rng(seed)
    f = rng.normal(0.0, 1.0, (h, w, 4)).astype(np.float16)
    f[rng.integers(0, 8, (h, w)) == 0, :3] = 0
    f[..., 3] = 1
    return f.view(np.uint16)


def _settings(itw, fmt):
    if fmt == "bc7":
        return itw.bc7_profile("veryfast")
    if fmt == "bc6h":
        return itw.bc6h_profile("fast")
    if fmt == "etc1":
        return itw.EtcSettings(1)
    return None


def _dev(gpu, a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(gpu)


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def _chains(itw, fmt):
    make = _rgba16f if fmt == "bc6h" else _rgba8
    return {"20x12 with mips": itw.mip_chain(make(12, 20, 1)), "16^2 cube with mips": [lv for f in range(6) for lv in itw.mip_chain(make(16, 16, 10 + f))]}


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("fmt,ops_list", [("bc1", (4, 3, 7)), ("bc5", (1, 4, 7)), ("bc7", (4, 7)), ("etc1", (7,)), ("bc6h", (7, 2))])
def test_chain_stream_is_the_plain_chain_of_prepared_copies(itw, gpu, fmt, ops_list, where):
    import torch
    for name, levels in _chains(itw, fmt).items():
        assert levels[-1].shape[:2] == (1, 1)
        for ops in ops_list:
            prepared = [N.prepare(lv, ops) for lv in levels]
            src = [_dev(gpu, lv) for lv in levels] if where == "device" else [lv.copy() for lv in levels]
            ok, want = itw.compress_chain(fmt, [_dev(gpu, p) for p in prepared] if where == "device" else prepared, settings=_settings(itw, fmt))
            assert ok
            ok, got = itw.compress_chain(fmt, src, settings=_settings(itw, fmt), normal_ops=ops)
            torch.cuda.synchronize()
            assert ok and np.array_equal(_np(got), _np(want)), (name, ops)
            for s, lv in zip(src, levels):
                assert np.array_equal(_np(s).view(lv.dtype), lv), "a source was written"
    # ops 0: the plain call's bytes
    levels = _chains(itw, fmt)["20x12 with mips"]
    src = [_dev(gpu, lv) for lv in levels] if where == "device" else levels
    a = itw.compress_chain(fmt, src, settings=_settings(itw, fmt), normal_ops=0)[1]
    b = itw.compress_chain(fmt, src, settings=_settings(itw, fmt))[1]
    assert np.array_equal(_np(a), _np(b))


@pytest.mark.parametrize("fmt,size", [("bc5", 2048), ("bc7", 1536)])
def test_an_image_the_plain_call_encodes_in_place_goes_through_the_gather(itw, gpu, fmt, size):
    """A window or more of blocks, multiples of 4: the plain call launches on the source itself; with ops the gather copies and prepares it."""
    import torch
    img = _rgba8(size, size, size)
    assert (size // 4) ** 2 >= (262144 if fmt == "bc5" else 131072)
    t = _dev(gpu, img)
    ok, want = itw.compress_chain(fmt, [_dev(gpu, N.prepare_rgba8(img, 4))], settings=_settings(itw, fmt))
    assert ok
    ok, got = itw.compress_chain(fmt, [t], settings=_settings(itw, fmt), normal_ops=4)
    torch.cuda.synchronize()
    assert ok and torch.equal(got, want)
    assert np.array_equal(t.cpu().numpy(), img)


def test_progress_and_the_early_out_are_the_plain_calls(itw, gpu):
    levels = [lv for f in range(6) for lv in itw.mip_chain(_rgba8(64, 64, 40 + f))]
    n = len(levels)
    src = [_dev(gpu, lv) for lv in levels]
    ok, want = itw.compress_chain("bc5", [_dev(gpu, N.prepare_rgba8(lv, 7)) for lv in levels])
    want = want.cpu().numpy()
    calls = []
    ok, got = itw.compress_chain("bc5", src, normal_ops=7, progress=lambda i, t, u: calls.append((i, t)) or True)
    assert ok and calls == [(i, n) for i in range(1, n + 1)] and np.array_equal(got.cpu().numpy(), want)
    k = n // 2
    calls = []

    def stop_at_k(i, t, u):
        calls.append(i)
        return i != k

    ok, got = itw.compress_chain("bc5", src, normal_ops=7, progress=stop_at_k)
    assert ok is False and calls == list(range(1, k + 1))
    written = sum(((lv.shape[0] + 3) // 4) * ((lv.shape[1] + 3) // 4) * 16 for lv in levels[:k - 1])
    assert np.array_equal(got.cpu().numpy()[:written], want[:written])


@pytest.mark.parametrize("face,vertical", [(8, False), (8, True), (5, False), (5, True)])
def test_cross_views_encode_and_decode_like_copied_faces(itw, gpu, face, vertical):
    import torch
    h, w = (4 * face, 3 * face) if vertical else (3 * face, 4 * face)
    cross = _rgba8(h, w, face + vertical)
    tc = _dev(gpu, cross)
    views = itw.cube_cross_faces(tc)
    copies = [v.contiguous() for v in views]
    assert all(v.shape[:2] == (face, face) for v in views) and views[0].data_ptr() != copies[0].data_ptr()
    for fmt, ops in (("bc7", None), ("bc5", 7)):
        kw = {} if ops is None else {"normal_ops": ops}
        ok, a = itw.compress_chain(fmt, views, settings=_settings(itw, fmt), **kw)
        ok2, b = itw.compress_chain(fmt, copies, settings=_settings(itw, fmt), **kw)
        torch.cuda.synchronize()
        assert ok and ok2 and torch.equal(a, b), (fmt, ops)
        assert np.array_equal(tc.cpu().numpy(), cross)
    # the inverse: the stream decoded into the cells of a canvas is what the decoder gives for six separate faces
    ok, stream = itw.compress_chain("bc7", views, settings=_settings(itw, "bc7"))
    canvas = torch.zeros_like(tc)
    itw.decode_chain("bc7", stream, itw.cube_cross_faces(canvas))
    separate = itw.decode_chain("bc7", stream, [(face, face)] * 6)
    torch.cuda.synchronize()
    for cell, img in zip(itw.cube_cross_faces(canvas), separate):
        assert torch.equal(cell, img)
    outside = canvas.clone()
    for cell in itw.cube_cross_faces(outside):
        cell.fill_(0)
    assert not outside.any() and canvas.any()
