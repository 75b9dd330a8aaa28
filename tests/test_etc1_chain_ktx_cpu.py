"""ETC1 above the block call, without a GPU: what the dispatch layer refuses before any device work (include/itw_dispatch.h), itwChainBytes
for ETC1's 8-byte blocks, and the KTX 1.1 container (the itwKtx* functions of include/itw_dds.h) field by field against a parser written here from the layout.

Mixed host and device images cannot be made without a device; that refusal is in tests/test_gpu_etc1_chain.py."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ETC1 = 0x8D64
KTX_ID = bytes([0xAB, 0x4B, 0x54, 0x58, 0x20, 0x31, 0x31, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A])
FIELDS = ("endianness", "glType", "glTypeSize", "glFormat", "glInternalFormat", "glBaseInternalFormat", "pixelWidth", "pixelHeight",
          "pixelDepth", "numberOfArrayElements", "numberOfFaces", "numberOfMipmapLevels", "bytesOfKeyValueData")


# ---- the dispatch layer ---------------------------------------------------------------------------------------------------------------------
def test_chain_bytes_counts_8_bytes_per_block(itw):
    L = itw.lib()
    rng = np.random.default_rng(5)
    lists = [[(1, 1)], [(3, 2)], [(29, 37)], [(64, 64)] * 6] + [[(int(h), int(w)) for h, w in rng.integers(1, 3000, size=(9, 2))] for _ in range(8)]
    for sizes in lists:
        arr = (itw.RgbaSurface * len(sizes))(*[itw.RgbaSurface(None, w, h, 4 * w) for h, w in sizes])
        want = 8 * sum(((h + 3) // 4) * ((w + 3) // 4) for h, w in sizes)
        assert L.itwChainBytes(C.cast(arr, C.c_void_p), len(sizes), ETC1) == want, sizes[:3]
        assert itw.chain_bytes("etc1", sizes) == want
    assert itw.chain_bytes("etc1", itw.mip_chain(np.zeros((29, 37, 4), np.uint8))) == 109 * 8
    bad = (itw.RgbaSurface * 2)(itw.RgbaSurface(None, 4, 4, 16), itw.RgbaSurface(None, 0, 4, 16))
    assert L.itwChainBytes(C.cast(bad, C.c_void_p), 2, ETC1) == -1 and L.itwChainBytes(None, 1, ETC1) == -1
    assert L.GetBytesPerBlock(ETC1) == 8


def test_slice_window_takes_the_heavy_formats_131072_blocks(itw):
    L = itw.lib()
    st = itw.etc_profile("slow")
    sp = C.cast(C.byref(st), C.c_void_p)
    # 4096^2 in 64 slices of 16 384 blocks: 8 slices make 131 072 blocks, as for BC7 `basic`; BC1 takes 16
    assert L.itwSliceWindowFor(ETC1, sp, 4096, 4096, 0x40000) == 8 == L.itwSliceWindow(ETC1, 4096, 4096, 0x40000)
    assert L.itwSliceWindow(98, 4096, 4096, 0x40000) == 8 and L.itwSliceWindow(71, 4096, 4096, 0x40000) == 16
    assert L.itwSliceWindowFor(ETC1, None, 256, 256, 4096) == 16      # the whole surface is below a window: all 16 slices


def test_bad_etc1_calls_return_false_before_any_device_use():
    """Null settings, a threshold below 1 and the chain's own argument rules, through every entry point that takes the format.  Run in a
    fresh interpreter: the error mode is process-wide."""
    code = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
import itw_amd
L = itw_amd.lib()
itw_amd.set_error_mode(itw_amd.ON_ERROR_RETURN)
ETC1 = 0x8D64
img = np.zeros((8, 8, 4), dtype=np.uint8)
out = np.full(4096, 0xA5, dtype=np.uint8)
def arr(*s):
    return C.cast((itw_amd.RgbaSurface * len(s))(*s), C.c_void_p)
def sp(t):
    s = itw_amd.EtcSettings(t)
    return s, C.cast(C.byref(s), C.c_void_p)
good = itw_amd.RgbaSurface(img.ctypes.data, 8, 8, 32)
keep, ok6 = sp(6)
keep0, zero = sp(0)
keepn, neg = sp(-3)
chain = {
    "null settings": (arr(good), 1, None, "settings"),
    "threshold 0": (arr(good), 1, zero, "fastSkipTreshold"),
    "threshold -3": (arr(good), 1, neg, "fastSkipTreshold"),
    "count 0": (arr(good), 0, ok6, ""),
    "null images": (None, 1, ok6, ""),
    "0-width image": (arr(good, itw_amd.RgbaSurface(img.ctypes.data, 0, 8, 32)), 2, ok6, ""),
    "null texels": (arr(itw_amd.RgbaSurface(None, 8, 8, 32)), 1, ok6, ""),
    "stride below the row": (arr(itw_amd.RgbaSurface(img.ctypes.data, 8, 8, 31)), 1, ok6, ""),
}
for name, (images, count, settings, word) in chain.items():
    L.itwClearError()
    ok = L.itwCompressImageChainEx(images, count, out.ctypes.data, ETC1, settings, None, None)
    err = itw_amd.last_error()
    assert ok is False and err and word in err, (name, ok, err)
L.itwClearError()
assert L.itwCompressImageChainEx(arr(good), 1, None, ETC1, ok6, None, None) is False and itw_amd.last_error()
# a caller's function: the chain's own rules are checked before it is ever called
called = []
fn = itw_amd.abi.COMPRESSION_FUNC(lambda s, o: called.append(1))
for name in ("count 0", "null images", "0-width image", "null texels", "stride below the row"):
    images, count, _, _ = chain[name]
    L.itwClearError()
    assert L.itwCompressImageChain(images, count, out.ctypes.data, C.cast(fn, C.c_void_p), ETC1, None, None) is False and itw_amd.last_error(), name
assert not called
# the slice pipeline
for name, settings, word in (("null settings", None, "settings"), ("threshold 0", zero, "fastSkipTreshold"), ("threshold -3", neg, "fastSkipTreshold")):
    L.itwClearError()
    ok = L.itwCompressImageSlicedEx(C.byref(good), out.ctypes.data, 16, ETC1, settings, 16, None, None)
    err = itw_amd.last_error()
    assert ok is False and err and word in err, (name, ok, err)
L.itwClearError()
assert L.itwCompressImageSlicedEx(C.byref(good), out.ctypes.data, 32, ETC1, ok6, 16, None, None) is False      # 2 blocks of 8 bytes per row: 16
assert "block_row_pitch" in itw_amd.last_error()
L.itwClearError()
assert L.itwCompressImageSlicedEx(None, out.ctypes.data, 16, ETC1, ok6, 16, None, None) is False and itw_amd.last_error()
assert (out == 0xA5).all()
# the refined calls keep refusing the format, and a PSNR has no ETC1 target
st = itw_amd.RefineStats()
L.itwClearError()
assert L.itwCompressImageRefined(C.byref(good), out.ctypes.data, ETC1, ok6, ok6, 7, 0, C.addressof(st), C.sizeof(st), None, None) is False
assert "one encoder" in itw_amd.last_error()
assert itw_amd.psnr_to_total_sse("etc1", 64, 64, 40.0) == 2 ** 64 - 1
print("rejected", len(chain))
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "rejected 8"


# ---- KTX 1.1 ----------------------------------------------------------------------------------------------------------------------------------
def parse_ktx(data):
    """The file's header as a dict and its images as [(level, face, width, height, offset, bytes)], from the layout alone."""
    data = bytes(data)
    assert data[:12] == KTX_ID
    hdr = dict(zip(FIELDS, struct.unpack_from("<13I", data, 12)))
    pos = 64 + hdr["bytesOfKeyValueData"]
    images = []
    for level in range(max(1, hdr["numberOfMipmapLevels"])):
        w, h = max(1, hdr["pixelWidth"] >> level), max(1, hdr["pixelHeight"] >> level)
        n = ((w + 3) // 4) * ((h + 3) // 4) * 8
        (image_size,) = struct.unpack_from("<I", data, pos)
        assert image_size == n, (level, image_size, n)
        pos += 4
        for face in range(hdr["numberOfFaces"]):
            images.append((level, face, w, h, pos, n))
            pos += n
    assert pos == len(data)
    return hdr, images


def _levels(width, height, mips, faces, seed=0):
    """Distinct bytes per image, KTX order."""
    rng = np.random.default_rng(seed)
    out = []
    for level in range(mips):
        w, h = max(1, width >> level), max(1, height >> level)
        for _ in range(faces):
            out.append(rng.integers(0, 256, ((w + 3) // 4) * ((h + 3) // 4) * 8, dtype=np.uint8))
    return out


CASES = {"2d": (64, 48, 1, False), "2d 37x29 full chain": (37, 29, 6, False), "cube 16 with mips": (16, 16, 5, True), "1x1": (1, 1, 1, False)}


@pytest.mark.parametrize("case", list(CASES))
def test_ktx_write_field_by_field_and_image_offsets_tile_the_file(itw, case):
    width, height, mips, cube = CASES[case]
    faces = 6 if cube else 1
    levels = _levels(width, height, mips, faces)
    data = itw.ktx_file(width, height, levels, mip_levels=mips, cubemap=cube)
    hdr, images = parse_ktx(data)
    assert hdr == {"endianness": 0x04030201, "glType": 0, "glTypeSize": 1, "glFormat": 0, "glInternalFormat": 0x8D64, "glBaseInternalFormat": 0x1907,
                   "pixelWidth": width, "pixelHeight": height, "pixelDepth": 0, "numberOfArrayElements": 0, "numberOfFaces": faces,
                   "numberOfMipmapLevels": mips, "bytesOfKeyValueData": 0}
    assert len(images) == mips * faces == len(levels)
    for (level, face, w, h, off, n), blocks in zip(images, levels):                   # level major, then face
        assert np.array_equal(data[off:off + n], blocks), (level, face)
    L = itw.lib()
    desc = itw.KtxDesc()
    assert L.itwKtxReadHeader(data.ctypes.data, data.size, C.byref(desc)) == 64
    assert (desc.width, desc.height, desc.mip_levels, desc.gl_internal_format, desc.is_cubemap, desc.key_value_bytes) == (width, height, mips, ETC1, int(cube), 0)
    assert L.itwKtxHeaderBytes(C.byref(desc)) == 64 and L.itwKtxFileBytes(C.byref(desc)) == data.size
    got = itw.ktx_images(desc)
    assert got == [(h, w, off, n) for _, _, w, h, off, n in images]
    # the images and the size words tile the file exactly
    at = 64
    for i, (h, w, off, n) in enumerate(got):
        if i % faces == 0:
            at += 4
        assert off == at
        at += n
    assert at == data.size
    assert L.itwKtxImage(C.byref(desc), len(got), None, None, None) == 0
    head = np.zeros(64, np.uint8)
    assert L.itwKtxWriteHeader(C.byref(desc), head.ctypes.data, 64) == 64 and np.array_equal(head, data[:64])
    assert L.itwKtxWriteHeader(C.byref(desc), head.ctypes.data, 63) == 0


def test_ktx_key_value_data_is_skipped_and_counted(itw):
    levels = _levels(37, 29, 6, 1, seed=1)
    plain = itw.ktx_file(37, 29, levels, mip_levels=6).tobytes()
    entry = b"KTXorientation\0S=r,T=d\0"
    kv = struct.pack("<I", len(entry)) + entry + b"\0" * (-len(entry) % 4)
    assert len(kv) % 4 == 0
    data = np.frombuffer(plain[:60] + struct.pack("<I", len(kv)) + kv + plain[64:], dtype=np.uint8)
    hdr, images = parse_ktx(data)
    assert hdr["bytesOfKeyValueData"] == len(kv)
    desc = itw.KtxDesc()
    assert itw.lib().itwKtxReadHeader(data.ctypes.data, data.size, C.byref(desc)) == 64 + len(kv)
    assert desc.key_value_bytes == len(kv) and itw.lib().itwKtxFileBytes(C.byref(desc)) == data.size
    assert itw.ktx_images(desc) == [(h, w, off, n) for _, _, w, h, off, n in images]
    for (h, w, off, n), blocks in zip(itw.ktx_images(desc), levels):
        assert np.array_equal(data[off:off + n], blocks)
    # what this library writes carries none
    out = np.zeros(data.size, np.uint8)
    ptrs = (C.c_void_p * len(levels))(*[lv.ctypes.data for lv in levels])
    assert itw.lib().itwKtxWriteFile(C.byref(desc), ptrs, len(levels), out.ctypes.data, out.size) == 0
    assert itw.lib().itwKtxWriteHeader(C.byref(desc), out.ctypes.data, out.size) == 0


def test_ktx_level_count_0_reads_as_1(itw):
    data = itw.ktx_file(20, 12, _levels(20, 12, 1, 1)).copy()
    data[56:60] = 0
    desc = itw.KtxDesc()
    assert itw.lib().itwKtxReadHeader(data.ctypes.data, data.size, C.byref(desc)) == 64 and desc.mip_levels == 1
    assert len(itw.ktx_images(desc)) == 1


def _patched(data, offset, value):
    out = data.copy()
    out[offset:offset + 4] = np.frombuffer(struct.pack("<I", value), dtype=np.uint8)
    return out


def test_ktx_refusals(itw):
    L = itw.lib()
    desc = itw.KtxDesc()

    def reads(d):
        d = np.ascontiguousarray(d)
        return L.itwKtxReadHeader(d.ctypes.data, d.size, C.byref(desc))

    flat = itw.ktx_file(37, 29, _levels(37, 29, 6, 1), mip_levels=6)
    cube = itw.ktx_file(16, 16, _levels(16, 16, 5, 6), mip_levels=5, cubemap=True)
    assert reads(flat) == 64 and reads(cube) == 64
    swapped = flat.copy()
    for word in range(13):                                                           # the whole header in the other byte order
        swapped[12 + 4 * word:16 + 4 * word] = flat[12 + 4 * word:16 + 4 * word][::-1]
    bad = {
        "identifier": _patched(flat, 4, 0x30322058),
        "other byte order": swapped,
        "endianness word alone": _patched(flat, 12, 0x01020304),
        "array": _patched(flat, 48, 2),
        "depth": _patched(flat, 44, 1),
        "ETC2": _patched(flat, 28, 0x9274),
        "RGBA8": _patched(flat, 28, 0x8058),
        "1D (height 0)": _patched(flat, 40, 0),
        "width 0": _patched(flat, 36, 0),
        "2 faces": _patched(flat, 52, 2),
        "non-square cube": _patched(cube, 40, 8),
        "33 levels": _patched(flat, 56, 33),
        "level 0 size word": _patched(flat, 64, 8 * 80 + 8),
        "level 3 size word": _patched(flat, parse_ktx(flat)[1][3][4] - 4, 16),
        "cube size word holds the level": _patched(cube, 64, 6 * 128),
        "truncated by a byte": flat[:-1],
        "header only": flat[:64],
        "63 bytes": flat[:63],
    }
    for name, data in bad.items():
        assert reads(data) == 0, name
    assert L.itwKtxReadHeader(None, 64, C.byref(desc)) == 0 and L.itwKtxReadHeader(flat.ctypes.data, flat.size, None) == 0
    with pytest.raises(ValueError):
        itw.load_ktx(bad["ETC2"])
    # descriptions this library does not store
    for d in (itw.KtxDesc(16, 8, 1, ETC1, 1, 0), itw.KtxDesc(16, 16, 1, 98, 0, 0), itw.KtxDesc(0, 16, 1, ETC1, 0, 0), itw.KtxDesc(16, 16, 0, ETC1, 0, 0),
              itw.KtxDesc(16, 16, 33, ETC1, 0, 0)):
        assert L.itwKtxHeaderBytes(C.byref(d)) == 0 and L.itwKtxFileBytes(C.byref(d)) == 0 and L.itwKtxImage(C.byref(d), 0, None, None, None) == 0
    assert L.itwKtxHeaderBytes(None) == 0
    with pytest.raises(ValueError):
        itw.ktx_file(16, 16, _levels(16, 16, 2, 1), mip_levels=3)                   # a level short
    ok = itw.KtxDesc(16, 16, 1, ETC1, 0, 0)
    blocks = np.zeros(128, np.uint8)
    ptrs = (C.c_void_p * 1)(blocks.ctypes.data)
    out = np.zeros(64 + 4 + 128, np.uint8)
    assert L.itwKtxWriteFile(C.byref(ok), ptrs, 1, out.ctypes.data, out.size) == out.size
    assert L.itwKtxWriteFile(C.byref(ok), ptrs, 1, out.ctypes.data, out.size - 1) == 0
    assert L.itwKtxWriteFile(C.byref(ok), ptrs, 2, out.ctypes.data, out.size) == 0
    assert L.itwKtxWriteFile(C.byref(ok), (C.c_void_p * 1)(None), 1, out.ctypes.data, out.size) == 0


def test_ktx_symbols_are_declared_and_bound(itw):
    with open(os.path.join(ROOT, "include", "itw_dds.h")) as f:
        header = f.read()
    for name in ("itwKtxHeaderBytes", "itwKtxFileBytes", "itwKtxWriteHeader", "itwKtxReadHeader", "itwKtxWriteFile", "itwKtxImage"):
        assert name in header and name in itw.EXPORTED_SYMBOLS and hasattr(itw.lib(), name)
    assert C.sizeof(itw.KtxDesc) == 24
