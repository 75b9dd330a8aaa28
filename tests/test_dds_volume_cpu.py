"""The volume .dds container (include/itw_dds.h: ItwDdsDesc with is_cubemap = ITW_DDS_VOLUME, the depth in array_size) without a GPU: the
header words _EncodeDDSHeader writes for TEX_DIMENSION_TEXTURE3D, the round trip for legacy and DX10 formats, the level-major file order,
and the correction of itwDdsReadHeader, which no longer reads a volume header as a 2D texture.  Line numbers are DirectXTexDDS.cpp's unless a file is named."""
import ctypes as C
import struct

import numpy as np
import pytest

import _mip3d as M3

LEGACY = {"bc1": b"DXT1", "bc1a": b"DXT1", "bc2": b"DXT3", "bc3": b"DXT5", "bc3_dxtex": b"DXT5", "bc4": b"BC4U", "bc4_snorm": b"BC4S", "bc5": b"BC5U", "bc5_snorm": b"BC5S"}
DX10 = {"bc1_srgb": 72, "bc1a_srgb": 72, "bc2_srgb": 75, "bc3_srgb": 78, "bc3_dxtex_srgb": 78, "bc6h": 95, "bc6h_sf16": 96, "bc7": 98, "bc7_srgb": 99}
READS_BACK = {"bc1a": "bc1", "bc1a_srgb": "bc1_srgb", "bc3_dxtex": "bc3", "bc3_dxtex_srgb": "bc3_srgb"}      # as the 2D reader reports them


def _words(raw, n):
    return struct.unpack("<%dI" % n, bytes(raw[:4 * n]))


def _header(itw, fmt, w, h, d, levels):
    desc = itw.DdsVolumeDesc(w, h, d, levels, itw.DXGI_FORMAT[fmt])
    n = itw.lib().itwDdsHeaderBytes(C.byref(desc))
    buf = np.full(n + 8, 0xA5, np.uint8)
    assert itw.lib().itwDdsWriteHeader(C.byref(desc), buf.ctypes.data, n) == n and (buf[n:] == 0xA5).all()
    return desc, buf[:n]


@pytest.mark.parametrize("fmt", sorted(LEGACY) + sorted(DX10))
def test_header_words_by_value(itw, fmt):
    w, h, d, levels = 12, 20, 6, 5
    desc, raw = _header(itw, fmt, w, h, d, levels)
    dx10 = fmt in DX10
    assert len(raw) == (148 if dx10 else 128)
    word = _words(raw, len(raw) // 4)
    assert word[0] == 0x20534444 and word[1] == 124                                        # "DDS ", dwSize
    # dwFlags: DDS_HEADER_FLAGS_TEXTURE | _MIPMAP (:542) | _VOLUME (:593) | _LINEARSIZE (:615)
    assert word[2] == 0x00001007 | 0x00020000 | 0x00800000 | 0x00080000
    assert (word[3], word[4], word[6]) == (h, w, d)                                        # :595-597
    assert word[5] == itw.lib().itwDdsLevelBytes(itw.DXGI_FORMAT[fmt], w, h)               # the top level's slice pitch (:616)
    assert word[7] == levels                                                               # :549
    assert word[8:19] == (0,) * 11
    assert word[19] == 32 and word[20] == 4                                                # ddspf: dwSize, DDS_FOURCC
    assert raw[84:88].tobytes() == (b"DX10" if dx10 else LEGACY[fmt])
    assert word[22:27] == (0,) * 5
    assert word[27] == 0x00001000 | 0x00400008                                             # dwCaps: _TEXTURE | _MIPMAP (:552)
    assert word[28] == 0x00200000                                                          # dwCaps2: DDS_FLAGS_VOLUME (:594)
    assert word[29:32] == (0,) * 3
    if dx10:
        assert word[32:37] == (DX10[fmt], 4, 0, 1, 0)                                      # dxgiFormat, resourceDimension 4 (:633), miscFlag, arraySize (:652), miscFlags2
    # one level: no MIPMAP caps
    _, one = _header(itw, fmt, w, h, d, 1)
    assert _words(one, 32)[27] == 0x00001000 and _words(one, 32)[2] & 0x00020000


@pytest.mark.parametrize("fmt", sorted(LEGACY) + sorted(DX10))
def test_write_read_round_trip(itw, fmt):
    L = itw.lib()
    for w, h, d, levels in ((12, 20, 6, 5), (16, 16, 16, 5), (1, 1, 8, 4), (5, 3, 7, 1), (8, 8, 1, 4)):
        desc, raw = _header(itw, fmt, w, h, d, levels)
        back = itw.DdsDesc(9, 9, 9, 9, 9, 9)
        assert L.itwDdsReadHeader(raw.ctypes.data, raw.size, C.byref(back)) == raw.size
        # a volume, its depth in array_size: where the reader used to say "2D, one texture" for a legacy volume header
        assert (back.width, back.height, back.array_size, back.mip_levels, back.is_cubemap) == (w, h, d, levels, itw.DDS_VOLUME)
        assert back.dxgi_format == itw.DXGI_FORMAT[READS_BACK.get(fmt, fmt)]
        # truncated headers
        for cut in (0, 4, 127, raw.size - 1):
            assert L.itwDdsReadHeader(raw.ctypes.data, cut, C.byref(back)) == 0, cut


def test_what_the_volume_reader_refuses(itw):
    L = itw.lib()
    back = itw.DdsDesc()

    def reads(raw):
        return L.itwDdsReadHeader(raw.ctypes.data, raw.size, C.byref(back))

    _, legacy = _header(itw, "bc1", 8, 8, 4, 1)
    _, dx10 = _header(itw, "bc7", 8, 8, 4, 1)
    assert reads(legacy) == 128 and reads(dx10) == 148
    assert back.is_cubemap == itw.DDS_VOLUME and back.array_size == 4
    no_flag = legacy.copy()                                                       # without DDS_HEADER_FLAGS_VOLUME a legacy header is a 2D file (:323)
    no_flag[8:12] = np.frombuffer(struct.pack("<I", 0x000A1007), np.uint8)
    assert reads(no_flag) == 128 and (back.is_cubemap, back.array_size) == (0, 1)
    for raw, word, value in ((dx10, 2, 0x000A1007),                                # DX10 dimension 3D without the flag (:291)
                             (legacy, 6, 0), (dx10, 6, 0),                         # a depth of 0
                             (dx10, 33, 3), (dx10, 33, 2),                         # DX10 with another dimension
                             (dx10, 35, 2),                                        # arraySize > 1 (:294-296)
                             (dx10, 32, 28), (dx10, 32, 0x83F2),                   # a format that is not BCn; the library's own codes are in no file
                             (legacy, 0, 0x20534445), (legacy, 1, 100), (legacy, 21, 0x31545844 + 1)):
        bad = raw.copy()
        bad[4 * word:4 * word + 4] = np.frombuffer(struct.pack("<I", value), np.uint8)
        assert reads(bad) == 0, (word, hex(value))
    # arraySize 0 in a file reads as 1, mip count 0 as 1
    ok = dx10.copy()
    ok[4 * 35:4 * 35 + 4] = 0
    ok[4 * 7:4 * 7 + 4] = 0
    assert reads(ok) == 148 and back.mip_levels == 1 and (back.is_cubemap, back.array_size) == (itw.DDS_VOLUME, 4)
    # descriptions the writer refuses
    for bad in (itw.DdsVolumeDesc(0, 8, 4, 1, 71), itw.DdsVolumeDesc(8, 0, 4, 1, 71), itw.DdsVolumeDesc(8, 8, 0, 1, 71), itw.DdsVolumeDesc(8, 8, 4, 0, 71),
                itw.DdsVolumeDesc(8, 8, 4, 1, 74), itw.DdsVolumeDesc(8, 8, 4, 1, 28), itw.DdsVolumeDesc(8, 8, 4, 1, 0x8D64)):
        assert L.itwDdsHeaderBytes(C.byref(bad)) == 0 and L.itwDdsFileBytes(C.byref(bad)) == 0
        assert L.itwDdsImage(C.byref(bad), 0, None, None, None) == 0
    good = itw.DdsVolumeDesc(8, 8, 4, 1, 71)
    buf = np.zeros(256, np.uint8)
    assert L.itwDdsWriteHeader(C.byref(good), buf.ctypes.data, 127) == 0 and L.itwDdsWriteHeader(C.byref(good), None, 128) == 0 and not buf.any()


def test_every_2d_header_reads_and_writes_as_before_and_the_volume_flag_is_looked_at(itw):
    L = itw.lib()
    for fmt in sorted(set(LEGACY) | set(DX10)):
        for cube, array in ((False, 1), (True, 1), (False, 3), (True, 2)):
            d = itw.DdsDesc(20, 12, 3, itw.DXGI_FORMAT[fmt], int(cube), array)
            if cube:
                d.width = d.height = 16
            n = L.itwDdsHeaderBytes(C.byref(d))
            raw = np.zeros(n, np.uint8)
            assert L.itwDdsWriteHeader(C.byref(d), raw.ctypes.data, n) == n
            assert _words(raw, 8)[6] == 1 and not _words(raw, 8)[2] & 0x00800000          # dwDepth 1, no volume flag: the bytes the 2D writer always wrote
            back = itw.DdsDesc()
            assert L.itwDdsReadHeader(raw.ctypes.data, n, C.byref(back)) == n
            assert (back.width, back.height, back.mip_levels, back.is_cubemap, back.array_size) == (d.width, d.height, 3, int(cube), array)
            assert back.dxgi_format == itw.DXGI_FORMAT[READS_BACK.get(fmt, fmt)]
            raw[8:12] = np.frombuffer(struct.pack("<I", _words(raw, 3)[2] | 0x00800000), np.uint8)
            # DDS_HEADER_FLAGS_VOLUME (:323-328): a legacy header becomes a volume of dwDepth 1, a DX10 header of dimension 2D contradicts itself
            got = L.itwDdsReadHeader(raw.ctypes.data, n, C.byref(back))
            assert (got, back.is_cubemap, back.array_size) == (128, itw.DDS_VOLUME, 1) if n == 128 else got == 0


@pytest.mark.parametrize("fmt", ["bc1", "bc3_srgb", "bc4", "bc6h"])
def test_file_order_and_image_offsets(itw, fmt):
    L = itw.lib()
    bpb = itw.BYTES_PER_BLOCK["bc6h" if fmt == "bc6h" else fmt.replace("_srgb", "")]
    for w, h, d in ((12, 20, 6), (16, 16, 16), (5, 3, 7), (1, 8, 1), (2, 2, 2)):
        for levels in {1, 2, M3.levels_of(w, h, d)}:
            slices, want, at = [], [], None
            desc = itw.DdsVolumeDesc(w, h, d, levels, itw.DXGI_FORMAT[fmt])
            at = L.itwDdsHeaderBytes(C.byref(desc))
            for l in range(levels):
                lw, lh, ld = M3.level_size(w, h, d, l)
                n = ((lw + 3) // 4) * ((lh + 3) // 4) * bpb
                for z in range(ld):
                    slices.append(np.full(n, (17 * l + z + 1) & 0xFF, np.uint8))
                    want.append((lh, lw, l, z, at, n))
                    at += n
            assert itw.dds_volume_images(desc) == want and L.itwDdsFileBytes(C.byref(desc)) == at
            assert L.itwDdsImage(C.byref(desc), len(want), None, None, None) == 0
            data = itw.dds_volume_file(fmt, w, h, d, slices, levels)
            assert data.size == at
            for (lh, lw, l, z, off, n), s in zip(want, slices):
                assert np.array_equal(data[off:off + n], s), (l, z)
            # the payload is the chain calls' packed stream over the same slice list
            assert itw.chain_bytes(fmt, [(lh, lw) for lh, lw, *_ in want]) == at - want[0][4]
            # a slice too few, a slice too many, a null slice, a short buffer
            for bad in (slices[:-1], slices + [slices[-1]]):
                with pytest.raises(ValueError):
                    itw.dds_volume_file(fmt, w, h, d, bad, levels)
            ptrs = (C.c_void_p * len(slices))(*[s.ctypes.data for s in slices])
            out = np.zeros(at, np.uint8)
            assert L.itwDdsWriteFile(C.byref(desc), ptrs, len(slices), out.ctypes.data, at - 1) == 0
            assert L.itwDdsWriteFile(C.byref(desc), ptrs, len(slices), out.ctypes.data, at) == at and np.array_equal(out, data)
            ptrs[len(slices) - 1] = None
            assert L.itwDdsWriteFile(C.byref(desc), ptrs, len(slices), out.ctypes.data, at) == 0


def test_load_dds_names_the_volume_loader_and_truncated_files_are_refused(itw):
    slices = [np.zeros(8 * 4, np.uint8) for _ in range(4)] + [np.zeros(8, np.uint8) for _ in range(2)]
    data = itw.dds_volume_file("bc1", 8, 8, 4, slices, 2)
    with pytest.raises(ValueError, match="load_dds_volume"):
        itw.load_dds(data)
    with pytest.raises(ValueError, match="load_dds_volume"):
        itw.load_dds(data.tobytes())
    for cut in (data.size - 1, 128 + 8 * 4 * 4, 128, 100):
        with pytest.raises(ValueError, match="truncated|not a BCn volume"):
            itw.load_dds_volume(data[:cut])
    flat = itw.dds_file("bc1", 8, 8, [np.zeros(32, np.uint8)], 1)
    with pytest.raises(ValueError, match="not a BCn volume"):
        itw.load_dds_volume(flat)
