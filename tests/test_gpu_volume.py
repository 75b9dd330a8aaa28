"""The volume save and load paths on the device: itwCompressImageMippedEx with ITW_MIP_VOLUME (include/itw_dispatch.h) is the 3D mip chain followed by the
chain encoder over the slice list, its payload is a volume .dds file's (include/itw_dds.h), and the load path brings the file back to the
texels itwDecodeChain gives.  Every comparison is == on bytes."""
import ctypes as C

import numpy as np
import pytest

import _mip3d as M3

pytestmark = pytest.mark.gpu

# (format, texel kind, encoder options): one format per encoder family and texel kind
FORMATS = [("bc1", "rgba8", {}), ("bc3_srgb", "rgba8", {}), ("bc4", "rgba8", {}), ("bc2", "rgba8", {}), ("bc7", "rgba8", {"profile": "ultrafast"}),
           ("bc6h", "rgba16f", {"profile": "veryfast"})]


def _volume(kind, w, h, d, seed):
    if kind == "rgba8":
        return M3.seeded_byte_volume(d, h, w, seed)
    v = M3.seeded_half_volume(d, h, w, seed)
    return (v & 0x7FFF).astype(np.uint16)                          # BC6H_UF16 sources: no negative halves


def _dev(gpu, a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a.copy()).to(gpu)


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


@pytest.mark.parametrize("fmt,kind,opts", FORMATS, ids=[f[0] for f in FORMATS])
def test_compress_volume_equals_compress_chain_over_the_generated_slices(itw, gpu, fmt, kind, opts):
    import torch
    for (w, h, d, seed), filt, wrap, levels in (((12, 20, 6, 3), None, "", 0), ((16, 16, 8, 4), None, "", 0), ((16, 16, 8, 4), "cubic", "uvw", 3), ((5, 3, 7, 5), "point", "", 0)):
        vol = _volume(kind, w, h, d, seed)
        srgb = kind == "rgba8" and fmt.endswith("_srgb")
        chain = itw.generate_mips_3d(_dev(gpu, vol), levels=levels, filter=filt, wrap=wrap, srgb=srgb)
        slices = [lv[z] for lv in chain for z in range(lv.shape[0])]
        ok, want = itw.compress_chain(fmt, slices, **opts)
        seen = []
        ok2, got = itw.compress_volume(fmt, _dev(gpu, vol), levels=levels, filter=filt, wrap=wrap, srgb=srgb, progress=lambda i, n, u: seen.append((i, n)) or True, **opts)
        ok3, host = itw.compress_volume(fmt, vol.copy(), levels=levels, filter=filt, wrap=wrap, srgb=srgb, **opts)
        torch.cuda.synchronize()
        assert ok and ok2 and ok3, itw.last_error()
        assert np.array_equal(_np(got), _np(want)) and np.array_equal(host, _np(want)), (fmt, (w, h, d), filt)
        assert seen == [(i, len(slices)) for i in range(1, len(slices) + 1)]                    # the chain call's contract: 1 .. slices
        assert want.numel() == itw.chain_bytes(fmt, [tuple(s.shape[:2]) for s in slices])
        n = levels or M3.levels_of(w, h, d)
        desc = itw.DdsVolumeDesc(w, h, d, n, itw.DXGI_FORMAT[fmt])
        assert want.numel() == itw.lib().itwDdsFileBytes(C.byref(desc)) - itw.lib().itwDdsHeaderBytes(C.byref(desc))


@pytest.mark.parametrize("fmt,kind,opts", FORMATS, ids=[f[0] for f in FORMATS])
def test_the_volume_dds_loads_to_the_texels_decode_chain_gives_and_measures(itw, gpu, fmt, kind, opts):
    import torch
    w, h, d = 12, 20, 6
    vol = _volume(kind, w, h, d, 9)
    ok, blocks = itw.compress_volume(fmt, vol.copy(), **opts)
    assert ok
    n = M3.levels_of(w, h, d)
    sizes = [M3.level_size(w, h, d, l) for l in range(n)]
    images = itw.dds_volume_images(itw.DdsVolumeDesc(w, h, d, n, itw.DXGI_FORMAT[fmt]))
    at, parts = 0, []
    for _, _, _, _, _, nb in images:
        parts.append(blocks[at:at + nb])
        at += nb
    assert at == blocks.size
    data = itw.dds_volume_file(fmt, w, h, d, parts, n)
    with pytest.raises(ValueError, match="load_dds_volume"):
        itw.load_dds(data)
    flat = itw.decode_chain(fmt, blocks, [(lh, lw) for lw, lh, ld in sizes for _ in range(ld)])
    for device in (None, gpu):
        desc, levels, amin = itw.load_dds_volume(data if device is None else data.tobytes(), device=device)
        torch.cuda.synchronize()
        assert (desc.width, desc.height, desc.array_size, desc.mip_levels, desc.is_cubemap) == (w, h, d, n, itw.DDS_VOLUME) and len(amin) == len(flat)
        assert [tuple(lv.shape) for lv in levels] == [(ld, lh, lw, 4) for lw, lh, ld in sizes]
        i = 0
        for lv in levels:
            for z in range(lv.shape[0]):
                assert np.array_equal(_np(lv[z]), flat[i]), (fmt, device, i)
                i += 1
    # measure over the same slice list
    chain = itw.generate_mips_3d(vol.copy())
    slices = [lv[z] for lv in chain for z in range(lv.shape[0])]
    stats = itw.measure_chain(fmt, blocks, slices)
    assert len(stats) == len(slices)


def test_the_one_call_save_refuses_what_the_generation_refuses(itw, gpu):
    import torch
    vol = _dev(gpu, _volume("rgba8", 8, 8, 4, 1))
    itw.set_error_mode(itw.ON_ERROR_RETURN)
    try:
        slices = itw.abi._surfaces([vol[z] for z in range(4)])
        out = torch.full((4096,), 0x5A, dtype=torch.uint8, device=gpu)
        for flags, word in ((0x200, "ITW_MIP_RESIZE"), (0x1000, "ITW_MIP_MIRROR"), (0x30, "two filter bits"), (2, "unknown mip flag")):
            assert itw.lib().itwCompressImageMippedEx(C.cast(slices, C.c_void_p), 4, 0, 0, flags | itw.MIP_VOLUME, out.data_ptr(), 71, None, None, None) is False
            assert word in itw.last_error(), (flags, itw.last_error())
        torch.cuda.synchronize()
        assert bool((out == 0x5A).all())
    finally:
        itw.lib().itwClearError()
        itw.set_error_mode(itw.ON_ERROR_ABORT)
