"""BC2 in the DDS container (include/itw_dds.h) without a GPU: a descriptor names BC2 by the library's two codes (0x83F2 / 0x8C4E), the file
holds DXGI's own -- the legacy 'DXT3' FourCC, or a DX10 header with 74 / 75 --, and a header read back gives the two codes again; the
premultiplied spellings 'DXT2' / 'DXT4' read as BC2 / BC3 (DirectXTex's mapping).  74 / 75 as descriptor codes stay refused
(tests/test_decode_chain_args.py pins that)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BC2, BC2_SRGB = 0x83F2, 0x8C4E


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


@pytest.mark.parametrize("code,w,h,mips,cube,arr,fourcc,stored", [
    (BC2, 64, 64, 1, False, 1, b"DXT3", None), (BC2, 61, 75, 7, False, 1, b"DXT3", None), (BC2, 16, 16, 5, True, 1, b"DXT3", None),
    (BC2, 32, 16, 3, False, 4, b"DX10", 74), (BC2, 16, 16, 2, True, 2, b"DX10", 74),
    (BC2_SRGB, 64, 64, 1, False, 1, b"DX10", 75), (BC2_SRGB, 16, 16, 5, True, 1, b"DX10", 75), (BC2_SRGB, 8, 8, 1, False, 3, b"DX10", 75)])
def test_header_round_trips(itw, code, w, h, mips, cube, arr, fourcc, stored):
    d, buf = _hdr(itw, code, w, h, mips, cube, arr)
    assert buf.size == (128 if stored is None else 148)
    assert buf[84:88].tobytes() == fourcc
    # ddspf as DirectXTex's DDSPF_DXT3 / DDSPF_DX10 (DDS.h): size 32, DDS_FOURCC, the FourCC, then zeros
    assert buf[76:108].tobytes() == struct.pack("<II4s5I", 32, 4, fourcc, 0, 0, 0, 0, 0)
    assert struct.unpack_from("<I", buf, 20)[0] == ((w + 3) // 4) * ((h + 3) // 4) * 16          # linear size of the top level
    if stored is not None:
        assert struct.unpack_from("<5I", buf, 128) == (stored, 3, 4 if cube else 0, arr, 0)        # the file's own truth: DXGI 74 / 75
    off, back = _read(itw, buf)
    assert off == buf.size and _fields(back) == (w, h, mips, code, 1 if cube else 0, arr)           # the library's code again


def test_sizes_are_16_bytes_per_block(itw):
    L = itw.lib()
    for code in (BC2, BC2_SRGB):
        assert L.itwDdsLevelBytes(code, 61, 75) == 16 * 19 * 16 == L.itwDdsLevelBytes(77, 61, 75)
        assert L.itwDdsLevelBytes(code, 1, 1) == 16 and L.itwDdsLevelBytes(code, 0, 0) == 16
        for w, h, mips, cube, arr in ((64, 64, 7, False, 1), (61, 75, 3, True, 1), (16, 16, 5, True, 2)):
            d = itw.DdsDesc(w, h, mips, code, 1 if cube else 0, arr)
            same = itw.DdsDesc(w, h, mips, 78, 1 if cube else 0, arr)          # BC3_SRGB: 16 bytes per block, always DX10
            chain = sum(((max(1, w >> l) + 3) // 4) * ((max(1, h >> l) + 3) // 4) * 16 for l in range(mips)) * (6 if cube else 1) * arr
            assert L.itwDdsFileBytes(C.byref(d)) == L.itwDdsHeaderBytes(C.byref(d)) + chain
            if code == BC2_SRGB:
                assert L.itwDdsFileBytes(C.byref(d)) == L.itwDdsFileBytes(C.byref(same))


def test_image_offsets_of_a_mipped_cube(itw):
    L = itw.lib()
    for code, hdr in ((BC2, 128), (BC2_SRGB, 148)):
        d = itw.DdsDesc(16, 16, 5, code, 1, 1)
        imgs = itw.dds_images(d)
        assert len(imgs) == 30 and [im[:2] for im in imgs[:5]] == [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
        sizes = [256, 64, 16, 16, 16]
        at = hdr
        for i, (h, w, off, n) in enumerate(imgs):
            assert (off, n) == (at, sizes[i % 5]), (i, off, n)
            at += n
        assert at == L.itwDdsFileBytes(C.byref(d))
        same = itw.dds_images(itw.DdsDesc(16, 16, 5, 78, 1, 1))
        if hdr == 148:
            assert imgs == same
        assert L.itwDdsImage(C.byref(d), 30, None, None, None) == 0


def _legacy(fourcc, w=32, h=16, mips=1):
    """A legacy (no DX10) DDS header as DirectXTex writes it for a block format, with the given FourCC."""
    b = bytearray(128)
    struct.pack_into("<4sIIIIIII", b, 0, b"DDS ", 124, 0x000A1007, h, w, ((w + 3) // 4) * ((h + 3) // 4) * 16, 1, mips)
    struct.pack_into("<II4s", b, 76, 32, 4, fourcc)
    struct.pack_into("<I", b, 108, 0x1000)
    return np.frombuffer(bytes(b), dtype=np.uint8)


def _dx10(dxgi, w=32, h=16, mips=1, arr=1):
    b = bytearray(148)
    b[:128] = _legacy(b"DX10", w, h, mips).tobytes()
    struct.pack_into("<5I", b, 128, dxgi, 3, 0, arr, 0)
    return np.frombuffer(bytes(b), dtype=np.uint8)


def test_reads_of_legacy_and_dx10_headers(itw):
    for cc, want in ((b"DXT3", BC2), (b"DXT2", BC2), (b"DXT5", 77), (b"DXT4", 77), (b"DXT1", 71)):
        off, d = _read(itw, _legacy(cc))
        assert off == 128 and _fields(d) == (32, 16, 1, want, 0, 1), cc
    for dxgi, want in ((74, BC2), (75, BC2_SRGB), (77, 77), (78, 78)):
        off, d = _read(itw, _dx10(dxgi, arr=2))
        assert off == 148 and _fields(d) == (32, 16, 1, want, 0, 2), dxgi
    # what no file holds: the library's own codes, the typeless BC2 (73), another FourCC
    for buf in (_dx10(BC2), _dx10(BC2_SRGB), _dx10(73), _legacy(b"DXT6")):
        assert _read(itw, buf)[0] == 0
    # a DXT3 file's payload is walked with the descriptor the read gives
    off, d = _read(itw, _legacy(b"DXT3", 61, 75, 7))
    assert off == 128 and len(itw.dds_images(d)) == 7 and itw.dds_images(d)[0][2:] == (128, 16 * 19 * 16)


def test_74_and_75_as_descriptor_codes_stay_refused(itw):
    """The file holds them; a descriptor does not (the refusal tests/test_decode_chain_args.py pins for itwDdsImage holds for all of itwDds*)."""
    L = itw.lib()
    buf = np.zeros(256, dtype=np.uint8)
    for code in (74, 75):
        d = itw.DdsDesc(16, 16, 1, code, 0, 1)
        assert L.itwDdsLevelBytes(code, 16, 16) == 0 and L.itwDdsHeaderBytes(C.byref(d)) == 0 and L.itwDdsFileBytes(C.byref(d)) == 0
        assert L.itwDdsWriteHeader(C.byref(d), buf.ctypes.data, buf.size) == 0 and L.itwDdsImage(C.byref(d), 0, None, None, None) == 0
    assert not buf.any()


def test_whole_file_and_the_binding(itw):
    rng = np.random.default_rng(5)
    for key, w, h, mips, cube in (("bc2", 64, 64, 1, False), ("bc2", 61, 75, 7, False), ("bc2_srgb", 16, 16, 5, True)):
        faces = 6 if cube else 1
        levels = [rng.integers(0, 256, ((max(1, w >> l) + 3) // 4) * ((max(1, h >> l) + 3) // 4) * 16, dtype=np.uint8) for _ in range(faces) for l in range(mips)]
        f = itw.dds_file(key, w, h, levels, mip_levels=mips, cubemap=cube)
        off, d = _read(itw, f)
        assert off == (128 if key == "bc2" else 148) and d.dxgi_format == itw.DXGI_FORMAT[key]
        assert np.array_equal(f[off:], np.concatenate(levels))
        # the same payload behind BC3's header of the same shape: only the format fields differ
        g = itw.dds_file("bc3" if key == "bc2" else "bc3_srgb", w, h, levels, mip_levels=mips, cubemap=cube)
        assert g.size == f.size and np.array_equal(np.nonzero(f != g)[0], [87] if key == "bc2" else [128])


@pytest.mark.parametrize("key,mips,cube,arr", [("bc2_srgb", 1, False, 1), ("bc2_srgb", 9, True, 1), ("bc2", 4, False, 3)])
def test_dx10_headers_read_back_through_the_references_own_dds_definitions(itw, tmp_path, key, mips, cube, arr):
    """oracle/_ref/ref_dds_check (DirectXTex/DDS.h compiled unmodified) checks a DX10 header field by field; it knows DXT1, DXT5, BC4U, BC5U
    and DX10 by name, so the legacy DXT3 header is compared with DDSPF_DXT3's bytes in test_header_round_trips instead, and it reads
    headers only: it offers no file written by the reference's writer."""
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_dds_check")
    if not os.path.exists(exe):
        if not os.path.exists("/root/reference/3rdParty/DirectXTex/DirectXTex/DDS.h"):
            pytest.skip("oracle/_ref/ref_dds_check not prebuilt and /root/reference absent")
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle", "ref_build")], check=True)
    d, buf = _hdr(itw, itw.DXGI_FORMAT[key], 256, 128, mips=mips, cube=cube, arr=arr)
    path = tmp_path / "h.dds"
    buf.tofile(path)
    r = subprocess.run([exe, str(path), "DX10", "75" if key == "bc2_srgb" else "74", "256", "128", str(mips), "1" if cube else "0", str(arr)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
