"""The two BC3_DXTEX codes (0x83F3 / 0x8C4F, include/itw_dispatch.h) in the DDS container (include/itw_dds.h) without a GPU: a descriptor
may name them, the file holds what the stream is -- the header of 77 / 78, byte for byte: the legacy 'DXT5' FourCC for 0x83F3 without an
array, a DX10 header with 77 / 78 otherwise --, and a header read back says 77 / 78.  No file holds the codes themselves; KTX does not
know them."""
import ctypes as C
import struct

import numpy as np
import pytest

BC3DX, BC3DX_SRGB = 0x83F3, 0x8C4F


def _hdr(itw, code, w, h, mips=1, cube=False, arr=1):
    d = itw.DdsDesc(w, h, mips, code, 1 if cube else 0, arr)
    n = itw.lib().itwDdsHeaderBytes(C.byref(d))
    buf = np.zeros(max(n, 1), dtype=np.uint8)
    assert itw.lib().itwDdsWriteHeader(C.byref(d), buf.ctypes.data, buf.size) == n
    return d, buf[:n]


def _read(itw, buf):
    d = itw.DdsDesc()
    buf = np.ascontiguousarray(buf)
    off = itw.lib().itwDdsReadHeader(buf.ctypes.data, buf.size, C.byref(d))
    return off, d


def _fields(d):
    return (d.width, d.height, d.mip_levels, d.dxgi_format, d.is_cubemap, d.array_size)


@pytest.mark.parametrize("code,same,w,h,mips,cube,arr,fourcc,size", [
    (BC3DX, 77, 64, 64, 1, False, 1, b"DXT5", 128), (BC3DX, 77, 61, 75, 7, False, 1, b"DXT5", 128), (BC3DX, 77, 16, 16, 5, True, 1, b"DXT5", 128),
    (BC3DX, 77, 32, 16, 3, False, 4, b"DX10", 148), (BC3DX, 77, 16, 16, 2, True, 2, b"DX10", 148),
    (BC3DX_SRGB, 78, 64, 64, 1, False, 1, b"DX10", 148), (BC3DX_SRGB, 78, 16, 16, 5, True, 1, b"DX10", 148), (BC3DX_SRGB, 78, 8, 8, 1, False, 3, b"DX10", 148)])
def test_the_header_is_that_of_77_or_78_and_reads_back_as_such(itw, code, same, w, h, mips, cube, arr, fourcc, size):
    d, buf = _hdr(itw, code, w, h, mips, cube, arr)
    _, ref = _hdr(itw, same, w, h, mips, cube, arr)
    assert buf.size == size and buf[84:88].tobytes() == fourcc
    assert np.array_equal(buf, ref)                                                               # the header of 77 / 78, byte for byte
    assert struct.unpack_from("<I", buf, 20)[0] == ((w + 3) // 4) * ((h + 3) // 4) * 16          # linear size of the top level
    if size == 148:
        assert struct.unpack_from("<5I", buf, 128) == (same, 3, 4 if cube else 0, arr, 0)
    off, back = _read(itw, buf)
    assert off == buf.size and _fields(back) == (w, h, mips, same, 1 if cube else 0, arr)           # a file says what the stream is


def test_sizes_and_image_offsets_follow_77_and_78(itw):
    L = itw.lib()
    for code, same, hdr in ((BC3DX, 77, 128), (BC3DX_SRGB, 78, 148)):
        assert L.itwDdsLevelBytes(code, 61, 75) == 16 * 19 * 16 == L.itwDdsLevelBytes(same, 61, 75)
        assert L.itwDdsLevelBytes(code, 1, 1) == 16
        for w, h, mips, cube, arr in ((64, 64, 7, False, 1), (61, 75, 3, True, 1), (16, 16, 5, True, 2)):
            d, s = itw.DdsDesc(w, h, mips, code, 1 if cube else 0, arr), itw.DdsDesc(w, h, mips, same, 1 if cube else 0, arr)
            assert L.itwDdsFileBytes(C.byref(d)) == L.itwDdsFileBytes(C.byref(s)) and L.itwDdsHeaderBytes(C.byref(d)) == L.itwDdsHeaderBytes(C.byref(s))
            assert itw.dds_images(d) == itw.dds_images(s)
        d = itw.DdsDesc(16, 16, 5, code, 1, 1)
        imgs = itw.dds_images(d)
        assert len(imgs) == 30 and [im[:2] for im in imgs[:5]] == [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
        at = hdr
        for i, (h, w, off, n) in enumerate(imgs):
            assert (off, n) == (at, [256, 64, 16, 16, 16][i % 5]), (i, off, n)
            at += n
        assert at == L.itwDdsFileBytes(C.byref(d)) and L.itwDdsImage(C.byref(d), 30, None, None, None) == 0


def test_no_file_holds_the_codes_and_ktx_does_not_know_them(itw):
    b = bytearray(148)
    struct.pack_into("<4sIIIIIII", b, 0, b"DDS ", 124, 0x000A1007, 16, 32, 8 * 4 * 16, 1, 1)
    struct.pack_into("<II4s", b, 76, 32, 4, b"DX10")
    struct.pack_into("<I", b, 108, 0x1000)
    for code, want in ((BC3DX, 0), (BC3DX_SRGB, 0), (77, 148), (78, 148)):
        struct.pack_into("<5I", b, 128, code, 3, 0, 1, 0)
        off, d = _read(itw, np.frombuffer(bytes(b), dtype=np.uint8))
        assert off == want and (not want or d.dxgi_format == code), code
    for code in (BC3DX, BC3DX_SRGB):
        kd = itw.KtxDesc(8, 8, 1, code, 0, 0)
        assert itw.lib().itwKtxFileBytes(C.byref(kd)) == 0


def test_whole_file_and_the_binding(itw):
    rng = np.random.default_rng(5)
    for key, same, w, h, mips, cube in (("bc3_dxtex", "bc3", 64, 64, 1, False), ("bc3_dxtex", "bc3", 61, 75, 7, False), ("bc3_dxtex_srgb", "bc3_srgb", 16, 16, 5, True)):
        faces = 6 if cube else 1
        levels = [rng.integers(0, 256, ((max(1, w >> l) + 3) // 4) * ((max(1, h >> l) + 3) // 4) * 16, dtype=np.uint8) for _ in range(faces) for l in range(mips)]
        f = itw.dds_file(key, w, h, levels, mip_levels=mips, cubemap=cube)
        off, d = _read(itw, f)
        assert off == (128 if key == "bc3_dxtex" else 148) and d.dxgi_format == itw.DXGI_FORMAT[same]
        assert np.array_equal(f[off:], np.concatenate(levels))
        assert np.array_equal(f, itw.dds_file(same, w, h, levels, mip_levels=mips, cubemap=cube))        # the file of 77 / 78
