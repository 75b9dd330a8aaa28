"""itwPreviewBlocks / itwPreviewSurface (include/itw_decode.h) without a GPU: the refusals, which come before any device work; the numpy
restatement tests/_preview.py against literals typed in here from the reference's text (IntelPlugin.cpp:585-639, IntelPlugin.h:41-48), not
computed by the module; and the compiled kernels' resources (tools/kernel_resources.py, as tests/test_kernel_occupancy.py reads them)."""
import ctypes as C
import os

import numpy as np
import pytest

import _preview
from test_kernel_occupancy import BUILD, resources

FORMATS = (71, 72, 77, 78, 80, 83, 95, 98, 99, 0x8D64)
R, G, B, A = 0x04, 0x08, 0x10, 0x20
INF, NAN = float("inf"), float("nan")


def _view(itw, **kw):
    v = dict(width=8, height=8, x_offset=0, y_offset=0, zoom=1.0, options=0, matte_color=0, exposure=1.0)
    v.update(kw)
    return itw.PreviewView(v["width"], v["height"], v["x_offset"], v["y_offset"], v["zoom"], v["options"], v["matte_color"], v["exposure"], 0)


BAD_VIEWS = {
    "view width 0": dict(width=0), "view width 16385": dict(width=16385), "view height 0": dict(height=0), "view height 16385": dict(height=16385),
    "negative view width": dict(width=-8), "x offset past 2^30": dict(x_offset=2 ** 30 + 1), "x offset below -2^30": dict(x_offset=-2 ** 30 - 1),
    "y offset past 2^30": dict(y_offset=2 ** 30 + 1), "y offset below -2^30": dict(y_offset=-2 ** 30 - 1),
    "zoom 0": dict(zoom=0.0), "zoom -0": dict(zoom=-0.0), "negative zoom": dict(zoom=-1.0), "zoom inf": dict(zoom=INF), "zoom nan": dict(zoom=NAN),
}


def test_the_view_struct_is_the_headers(itw, tmp_path):
    import subprocess
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "itw_decode.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %g %d %d\\n", sizeof(itw_preview_view), offsetof(itw_preview_view, zoom), '
                   'offsetof(itw_preview_view, options), offsetof(itw_preview_view, exposure), (double)ITW_PREVIEW_TILE_MAX_ZOOM, '
                   'ITW_PREVIEW_CHANNEL_MASK, ITW_PREVIEW_CHANNEL_ALPHA); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(os.path.dirname(BUILD), "..", "..", "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    V = itw.PreviewView
    assert [int(v) for v in got[:4]] == [C.sizeof(V), V.zoom.offset, V.options.offset, V.exposure.offset] == [40, 16, 24, 32]
    assert float(got[4]) == itw.PREVIEW_TILE_MAX_ZOOM and int(got[5]) == itw.PREVIEW_CHANNEL_MASK == _preview.MASK
    assert int(got[6]) == itw.PREVIEW_CHANNEL["a"] == _preview.ALPHA


@pytest.mark.parametrize("fmt", FORMATS)
def test_preview_blocks_refuses_before_any_device_work(itw, fmt):
    L = itw.lib()
    blocks, out = np.zeros(4096, dtype=np.uint8), np.zeros(64 * 64 * 3, dtype=np.uint8)
    b, o, n = blocks.ctypes.data, out.ctypes.data, C.sizeof(itw.PreviewView)
    good = _view(itw)
    cases = {
        "null blocks": (None, 8, 8, C.byref(good), n, o, 24), "null view": (b, 8, 8, None, n, o, 24), "null out": (b, 8, 8, C.byref(good), n, None, 24),
        "view_bytes short": (b, 8, 8, C.byref(good), n - 4, o, 24), "view_bytes long": (b, 8, 8, C.byref(good), n + 8, o, 24),
        "view_bytes 0": (b, 8, 8, C.byref(good), 0, o, 24),
        "width 0": (b, 0, 8, C.byref(good), n, o, 24), "height 0": (b, 8, 0, C.byref(good), n, o, 24), "negative width": (b, -4, 8, C.byref(good), n, o, 24),
        "too many blocks": (b, 32768, 16388, C.byref(good), n, o, 24),
        "stride below the row": (b, 8, 8, C.byref(good), n, o, 23), "stride 0": (b, 8, 8, C.byref(good), n, o, 0), "negative stride": (b, 8, 8, C.byref(good), n, o, -24),
    }
    for name, kw in BAD_VIEWS.items():
        v = _view(itw, **kw)
        cases[name] = (b, 8, 8, C.byref(v), n, o, 3 * 16385)
    for name, args in cases.items():
        assert L.itwPreviewBlocks(fmt, *args) == -1, (fmt, name)
    assert not out.any()


@pytest.mark.parametrize("fmt", [81, 84, 96, 0, 28, 70, 73, 74, 82, 94, 97, 100, -1])
def test_preview_blocks_refuses_unknown_and_signed_formats(itw, fmt):
    """BC4S / BC5S (81, 84) and BC6H_SF16 (96): the reference previews neither, and an int8 viewport is not something it defines."""
    blocks, out = np.zeros(256, dtype=np.uint8), np.zeros(8 * 8 * 3, dtype=np.uint8)
    v = _view(itw)
    assert itw.lib().itwPreviewBlocks(fmt, blocks.ctypes.data, 8, 8, C.byref(v), C.sizeof(v), out.ctypes.data, 24) == -1
    assert not out.any()


@pytest.mark.parametrize("texel", [4, 8])
def test_preview_surface_refuses_before_any_device_work(itw, texel):
    L = itw.lib()
    S = itw.RgbaSurface
    texels, out = np.zeros(64 * 64 * texel, dtype=np.uint8), np.zeros(64 * 64 * 3, dtype=np.uint8)
    p, o, n = texels.ctypes.data, out.ctypes.data, C.sizeof(itw.PreviewView)
    good, src = _view(itw), S(p, 8, 8, 8 * texel)
    cases = {
        "null source": (None, texel, C.byref(good), n, o, 24), "null texels": (C.byref(S(None, 8, 8, 8 * texel)), texel, C.byref(good), n, o, 24),
        "null view": (C.byref(src), texel, None, n, o, 24), "null out": (C.byref(src), texel, C.byref(good), n, None, 24),
        "view_bytes short": (C.byref(src), texel, C.byref(good), n - 1, o, 24),
        "width 0": (C.byref(S(p, 0, 8, 8 * texel)), texel, C.byref(good), n, o, 24), "height 0": (C.byref(S(p, 8, 0, 8 * texel)), texel, C.byref(good), n, o, 24),
        "too many blocks": (C.byref(S(p, 32768, 16388, 32768 * texel)), texel, C.byref(good), n, o, 24),
        "source stride below its row": (C.byref(S(p, 8, 8, 8 * texel - 1)), texel, C.byref(good), n, o, 24),
        "stride below the row": (C.byref(src), texel, C.byref(good), n, o, 23),
    }
    for bad in (0, 1, 2, 3, 5, 12, 16, -4):
        cases[f"texel_bytes {bad}"] = (C.byref(src), bad, C.byref(good), n, o, 24)
    for name, kw in BAD_VIEWS.items():
        v = _view(itw, **kw)
        cases[name] = (C.byref(src), texel, C.byref(v), n, o, 3 * 16385)
    for name, args in cases.items():
        assert L.itwPreviewSurface(*args) == -1, (texel, name)
    assert not out.any()


# ---- tests/_preview.py against literals ------------------------------------------------------------------------------------------------

X = _preview.NONE
CHANNEL_TABLE = {   # mask: (byte 0, byte 1, byte 2), alpha alone -- IntelPlugin.cpp:585-624 read with planes = 4
    0:             ((0, 1, 2), False),          # no channel bit reads as RGB
    R:             ((0, 0, 0), False),
    G:             ((1, 1, 1), False),
    B:             ((2, 2, 2), False),
    A:             ((3, 3, 3), True),
    R | G:         ((0, 1, X), False),
    R | B:         ((0, X, 2), False),
    G | B:         ((X, 1, 2), False),
    R | G | B:     ((0, 1, 2), False),
    R | A:         ((0, X, 3), False),
    G | A:         ((X, 1, 3), False),
    B | A:         ((X, X, 3), False),          # alpha replaces blue
    R | G | A:     ((0, 1, 3), False),
    R | B | A:     ((0, X, 3), False),          # alpha replaces blue
    G | B | A:     ((X, 1, 3), False),          # alpha replaces blue
    R | G | B | A: ((0, 1, 3), False),          # alpha replaces blue
}


def test_the_channel_table_for_all_16_masks():
    assert len(CHANNEL_TABLE) == 16 and set(CHANNEL_TABLE) == {m << 2 for m in range(16)}
    for m, (ch, alone) in CHANNEL_TABLE.items():
        for other_bits in (0, 0x03, 0xFFFFFFC3):                 # bits outside the mask are ignored
            got, got_alone = _preview.channel_table(m | other_bits)
            assert (tuple(got), got_alone) == (ch, alone), hex(m)


def test_the_fraction_rule():
    """zoom 0.5, W = 10: xt + xo = -1 gives fx = -0.5 -> column 0; -2 gives fx = -1.0 -> outside; 20 gives fx = W -> outside; 19 -> column 9."""
    inside, x = _preview.coords(24, -3, 0.5, 10)                 # xt + xo = -3 .. 20
    assert inside.tolist() == [False, False] + [True] * 21 + [False]
    assert x[2:23].tolist() == [0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9]
    inside, x = _preview.coords(4, 2 ** 30, 1000.0, 16384)       # far beyond the int range: outside, never converted
    assert not inside.any()
    inside, x = _preview.coords(3, -1, 1.0, 1)                   # fx = -1, 0, 1 on a one-texel image
    assert inside.tolist() == [False, True, False] and x[1] == 0


def _half(x):
    return int(np.array([x], dtype=np.float16).view(np.uint16)[0])


def test_float_to_byte_at_its_edges():
    one_up = 0x3C01                                              # nextafter(1, 2) in half
    assert np.float16(1.0).view(np.uint16) == 0x3C00
    cases = [   # half bits, exposure, byte
        (0x0000, 1.0, 0), (0x8000, 1.0, 0),                      # 0, -0.0
        (0x3C00, 1.0, 255), (one_up, 1.0, 255),                  # 1 -> 255.0 -> 255; above 1 -> 255
        (0x3BFF, 1.0, 254),                                      # the half below 1: 0.99951171875 * 255 = 254.87...
        (0x7C00, 1.0, 255), (0xFC00, 1.0, 0),                    # inf, -inf
        (0x7E00, 1.0, 0), (0xFE00, 1.0, 0), (0x7C01, 1.0, 0),    # NaNs
        (0x7C00, 0.0, 0),                                        # inf * 0 = NaN
        (0xBC00, -1.0, 255), (0x3C00, -1.0, 0),                  # a negative exposure flips the sign
        (0x3800, 2.0, 255), (0x3800, 1.0, 127),                  # 0.5 * 2 = 1 -> 255; 0.5 * 255 = 127.5 -> 127
        (0x0001, 1.0, 0), (0x0001, INF, 255),                    # the smallest denormal
    ]
    # 1/255 and its neighbours: the halves around 0.00392156862745098 (0x1C04 = 0.003921508789..., 0x1C05 = 0.003925323486...)
    assert float(np.array([0x1C04], np.uint16).view(np.float16)[0]) * 255 < 1.0 < float(np.array([0x1C05], np.uint16).view(np.float16)[0]) * 255
    cases += [(0x1C03, 1.0, 0), (0x1C04, 1.0, 0), (0x1C05, 1.0, 1), (0x1C06, 1.0, 1)]
    for bits, exposure, want in cases:
        got = _preview.float_to_byte(np.array([bits], dtype=np.uint16), exposure)
        assert got.dtype == np.uint8 and int(got[0]) == want, (hex(bits), exposure, int(got[0]), want)
    assert _half(1.0) == 0x3C00 and _preview.float_to_byte(np.array([_half(0.25)], np.uint16), 1.0)[0] == 63      # 63.75 -> 63


def test_a_small_viewport_by_hand():
    """2 x 2 RGBA8 image, 4 x 3 view at offset (-1, -1), zoom 1, matte 0x00332211, channels R | A."""
    img = np.array([[[10, 20, 30, 40], [11, 21, 31, 41]], [[12, 22, 32, 42], [13, 23, 33, 43]]], dtype=np.uint8)
    got = _preview.viewport(img, 4, 3, -1, -1, 1.0, R | A, 0x00332211)
    m = [0x11, 0x22, 0x33]
    assert got.tolist() == [[m, m, m, m], [m, [10, 0, 40], [11, 0, 41], m], [m, [12, 0, 42], [13, 0, 43], m]]


# ---- the compiled kernels --------------------------------------------------------------------------------------------------------------

def test_every_preview_kernel_runs_without_scratch():
    """Picking texel px[ty * 4 + tx] out of the decoded block with an index that differs between lanes sends the array to scratch (80 - 144 B
    a lane when it happened): every instantiation has 0 B, the tile route has the LDS of 33 x 9 blocks and the per-pixel route none."""
    path = os.path.join(BUILD, "preview.o")
    if not os.path.exists(path):
        pytest.skip("csrc/build/ is not populated: run __graft_entry__.build() first")
    import re
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(BUILD), "..", "..", "tools", "kernel_resources.py"), path, "preview_kernel"],
                         check=True, capture_output=True, text=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"void itw::preview_kernel<(\d+), (true|false)>\s.*scratch\s+(\d+) B\s+lds\s+(\d+) B\s+spills v(\d+) s(\d+)", line)
        assert m, line
        seen[(int(m.group(1)), m.group(2) == "true")] = tuple(int(m.group(i)) for i in (3, 4, 5, 6))
    kinds = (1, 3, 4, 5, 6, 7, 20)                               # bc1, bc3, bc4, bc5, bc6h, bc7, etc1 (bcn_format.hpp)
    assert set(seen) == {(k, t) for k in kinds for t in (True, False)} | {(100, False), (101, False)}, sorted(seen)
    for (kind, tile), (scratch, lds, vspill, sspill) in seen.items():
        assert (scratch, vspill, sspill) == (0, 0, 0), (kind, tile, scratch, vspill, sspill)
        assert lds == ((33 * 9 * (96 if kind == 6 else 64)) if tile else 0), (kind, tile, lds)
    table = resources(path)                                      # and the occupancy both limits leave: at least 4 waves per SIMD
    for name, (regs, lds) in table.items():
        assert min(512 // (-(-regs // 8) * 8), (160 * 1024) // lds if lds else 8) >= 4, (name, regs, lds)
