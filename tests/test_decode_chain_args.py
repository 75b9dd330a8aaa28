"""The argument checks of itwDecodeChain / itwDecodeImage / itwDecodeBlocks (include/itw_decode.h) and itwDdsImage (include/itw_dds.h):
host-only, no GPU needed.

A refused call returns -1 BEFORE any device work, on a box without a GPU as on one with it; count == 0 returns 0.  (The one refusal
that needs a device pointer to state -- mixed host and device outputs -- is in tests/test_gpu_decode_chain.py.)"""
import ctypes as C

import numpy as np
import pytest

DECODED = (71, 72, 77, 78, 80, 81, 83, 84, 95, 98, 99)
WRITTEN = (71, 72, 77, 78, 80, 81, 83, 84, 95, 96, 98, 99)
MAX_BLOCKS = 33554432                                            # ITW_MEASURE_MAX_BLOCKS


def _arr(itw, *surfs):
    return C.cast((itw.RgbaSurface * len(surfs))(*surfs), C.c_void_p)


@pytest.mark.parametrize("fmt", DECODED)
def test_every_refusal_returns_minus_one(itw, fmt):
    L = itw.lib()
    S = itw.RgbaSurface
    px = 8 if fmt == 95 else 4
    texels = np.zeros(64 * 64 * px, dtype=np.uint8)
    blocks = np.zeros(4096, dtype=np.uint8)
    p, b = texels.ctypes.data, blocks.ctypes.data
    good = S(p, 8, 8, 8 * px)
    cases = {
        "count < 0": (b, _arr(itw, good), -1),
        "null blocks": (None, _arr(itw, good), 1),
        "null outs": (b, None, 1),
        "null texel pointer": (b, _arr(itw, good, S(None, 8, 8, 8 * px)), 2),
        "width 0": (b, _arr(itw, S(p, 0, 8, 8 * px)), 1),
        "height 0": (b, _arr(itw, good, S(p, 8, 0, 8 * px)), 2),
        "negative width": (b, _arr(itw, S(p, -4, 8, 8 * px)), 1),
        "stride below the row": (b, _arr(itw, S(p, 8, 8, 8 * px - 4)), 1),
        "stride not a multiple of 4": (b, _arr(itw, S(p, 7, 8, 7 * px + 2)), 1),
        "too many blocks in one image": (b, _arr(itw, S(p, 32768, 16388, 32768 * px)), 1),
    }
    assert (32768 // 4) * (16388 // 4) > MAX_BLOCKS
    for name, (bl, outs, count) in cases.items():
        assert L.itwDecodeChain(fmt, bl, outs, count, None, None) == -1, (fmt, name)
    for name in ("null blocks", "null outs", "width 0", "negative width", "stride below the row", "stride not a multiple of 4",
                 "too many blocks in one image"):
        bl, outs, _ = cases[name]
        assert L.itwDecodeImage(fmt, bl, outs, None, None) == -1, (fmt, name)
    # an empty chain is no error, whatever the pointers
    assert L.itwDecodeChain(fmt, b, _arr(itw, good), 0, None, None) == 0
    assert L.itwDecodeChain(fmt, None, None, 0, None, None) == 0


@pytest.mark.parametrize("fmt", [96, 0, 28, 70, 73, 74, 82, 94, 97, 100, -1])
def test_unknown_and_refused_formats(itw, fmt):
    """BC6H_SF16 (96) is refused: the signed decode is not built.  BC2 (74) and everything that is not a BCn format this library reads too."""
    L = itw.lib()
    texels = np.zeros(8 * 8 * 8, dtype=np.uint8)
    blocks = np.zeros(64, dtype=np.uint8)
    good = itw.RgbaSurface(texels.ctypes.data, 8, 8, 64)
    assert L.itwDecodeChain(fmt, blocks.ctypes.data, _arr(itw, good), 1, None, None) == -1
    assert L.itwDecodeChain(fmt, blocks.ctypes.data, _arr(itw, good), 0, None, None) == -1        # the format is checked first
    assert L.itwDecodeImage(fmt, blocks.ctypes.data, _arr(itw, good), None, None) == -1


# ---- itwDecodeBlocks: its own rules, all before any device work --------------------------------------------------------------------

WHOLE_BLOCKS = (71, 77, 95, 96, 98)                              # width and height must be multiples of 4
PARTIAL_BLOCKS = (80, 81, 83, 84)                                # BC4 / BC5, UNORM and SNORM: any size >= 1


def _decode_blocks(itw, fmt, w, h, stride, texels, blocks):
    return itw.lib().itwDecodeBlocks(fmt, blocks.ctypes.data, w, h, texels.ctypes.data, stride, None)


@pytest.mark.parametrize("fmt", WHOLE_BLOCKS + PARTIAL_BLOCKS + (72, 78, 99))
def test_decode_blocks_refuses_a_bad_stride(itw, fmt):
    px = 8 if fmt in (95, 96) else 4
    texels, blocks = np.zeros(16 * 16 * px, dtype=np.uint8), np.zeros(256, dtype=np.uint8)
    for stride, what in ((8 * px + 2, "not a multiple of 4"), (8 * px + 1, "odd"), (8 * px - 4, "below the row"), (0, "zero"),
                         (-8 * px, "negative"), (4, "one texel"), (2 ** 31, "more than an rgba_surface's stride holds")):
        assert _decode_blocks(itw, fmt, 8, 8, stride, texels, blocks) == -1, (fmt, what)
    assert not texels.any()


@pytest.mark.parametrize("fmt", WHOLE_BLOCKS)
def test_decode_blocks_refuses_partial_blocks_where_the_format_has_none(itw, fmt):
    px = 8 if fmt in (95, 96) else 4
    texels, blocks = np.zeros(16 * 16 * px, dtype=np.uint8), np.zeros(256, dtype=np.uint8)
    for w, h in ((6, 8), (8, 6), (0, 4), (4, 0), (3, 3), (-4, 4)):
        assert _decode_blocks(itw, fmt, w, h, 16 * px, texels, blocks) == -1, (fmt, w, h)
    assert not texels.any()


@pytest.mark.parametrize("fmt", WHOLE_BLOCKS + PARTIAL_BLOCKS)
def test_decode_blocks_refuses_more_blocks_than_one_launch_covers(itw, fmt):
    """46341^2 blocks > 2^31 - 1: refused, where the (int32_t) cast of the block count used to truncate.  The refusal comes before any
    pointer is looked at; the largest image that passes (46340^2 blocks, 128 GiB of RGBA8) is not something a test decodes."""
    px = 8 if fmt in (95, 96) else 4
    texels, blocks = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint8)
    side = 4 * 46341
    assert (side // 4) ** 2 > 2 ** 31 - 1 > (side // 4 - 1) ** 2 and side * px < 2 ** 31
    assert _decode_blocks(itw, fmt, side, side, side * px, texels, blocks) == -1
    assert not texels.any()


@pytest.mark.parametrize("fmt", PARTIAL_BLOCKS)
def test_decode_blocks_refuses_an_empty_surface(itw, fmt):
    texels, blocks = np.zeros(16 * 16 * 4, dtype=np.uint8), np.zeros(256, dtype=np.uint8)
    for w, h in ((0, 4), (4, 0), (-1, 4), (4, -1)):
        assert _decode_blocks(itw, fmt, w, h, 64, texels, blocks) == -1, (fmt, w, h)
    assert not texels.any()


@pytest.mark.parametrize("fmt", [0, 28, 70, 73, 74, 82, 94, 97, 100, -1])
def test_decode_blocks_refuses_an_unknown_format(itw, fmt):
    """(96, BC6H_SF16, is not among them: itwDecodeBlocks reads it as unsigned -- tests/test_gpu_decode_unified.py.)"""
    texels, blocks = np.zeros(8 * 8 * 8, dtype=np.uint8), np.zeros(64, dtype=np.uint8)
    assert _decode_blocks(itw, fmt, 8, 8, 64, texels, blocks) == -1
    assert not texels.any()


def _image(itw, d, i):
    w, h, off = C.c_uint32(0xdead), C.c_uint32(0xdead), C.c_size_t(0xdead)
    n = itw.lib().itwDdsImage(C.byref(d), i, C.byref(w), C.byref(h), C.byref(off))
    return int(n), int(w.value), int(h.value), int(off.value)


SHAPES = [  # width, height, mips, cube, array
    (37, 21, 1, 0, 1), (37, 21, 6, 0, 1), (1023, 517, 10, 0, 1), (16, 16, 5, 1, 1), (64, 64, 7, 1, 3), (5, 9, 4, 0, 4), (1, 1, 1, 0, 1),
    (4096, 4096, 13, 0, 1), (1, 7, 3, 0, 2),
]


@pytest.mark.parametrize("fmt", WRITTEN)
def test_dds_image_walks_the_payload(itw, fmt):
    L = itw.lib()
    for w0, h0, mips, cube, items in SHAPES:
        d = itw.DdsDesc(w0, h0, mips, fmt, cube, items)
        at = L.itwDdsHeaderBytes(C.byref(d))
        assert at in (128, 148)
        i = 0
        for _item in range(items * (6 if cube else 1)):
            w, h = w0, h0
            for _m in range(mips):
                n, gw, gh, off = _image(itw, d, i)
                assert (n, gw, gh, off) == (L.itwDdsLevelBytes(fmt, w, h), w, h, at), (fmt, w0, h0, mips, cube, items, i)
                at += n
                i += 1
                w, h = max(1, w // 2), max(1, h // 2)
        assert at == L.itwDdsFileBytes(C.byref(d))               # the last image ends where the file does
        for bad in (i, i + 1, 0xFFFFFFFF):
            assert _image(itw, d, bad) == (0, 0xdead, 0xdead, 0xdead)     # out of range: 0, nothing written
        assert L.itwDdsImage(C.byref(d), 0, None, None, None) == L.itwDdsLevelBytes(fmt, w0, h0)   # the outputs are optional


def test_dds_image_refuses_what_the_library_does_not_read(itw):
    L = itw.lib()
    assert L.itwDdsImage(None, 0, None, None, None) == 0
    for d in (itw.DdsDesc(16, 16, 1, 28, 0, 1), itw.DdsDesc(16, 16, 1, 74, 0, 1), itw.DdsDesc(0, 16, 1, 98, 0, 1),
              itw.DdsDesc(16, 16, 0, 98, 0, 1)):
        assert _image(itw, d, 0) == (0, 0xdead, 0xdead, 0xdead)


def test_the_binding_lists_a_files_images(itw):
    d = itw.DdsDesc(16, 16, 5, 77, 1, 1)
    imgs = itw.dds_images(d)
    assert len(imgs) == 30 and [im[:2] for im in imgs[:5]] == [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    assert imgs[0][2] == 128 and imgs[-1][2] + imgs[-1][3] == itw.lib().itwDdsFileBytes(C.byref(d))
