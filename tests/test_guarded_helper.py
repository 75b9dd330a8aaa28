"""tests/_guarded.py catches what it is for: numpy buffers only, no kernel involved."""
import numpy as np
import pytest

from _guarded import GUARD, GuardError, frozen, guarded, pattern, rows_of


def _fails_at(g, first, last, count):
    with pytest.raises(GuardError) as e:
        g.check("helper")
    assert (e.value.first, e.value.last, e.value.count) == (first, last, count), str(e.value)
    assert f"offsets {first} .. {last}" in str(e.value)


def test_the_pattern_is_position_dependent_and_fills_the_payload_too():
    g = guarded(1000)
    i = np.arange(g.buf.size)
    assert np.array_equal(g.buf, (i * 167 + 13) & 0xff)
    assert np.array_equal(pattern(300, start=77), ((np.arange(77, 377) * 167 + 13) & 0xff).astype(np.uint8))
    assert g.start >= GUARD and g.buf.size - g.start - 1000 >= GUARD and g.ptr == g.buf.ctypes.data + g.start
    assert g.view.size == 1000 and g.view.ctypes.data == g.ptr and g.ptr % 16 == 0
    assert (np.diff(g.buf.astype(np.int16)) != 0).all()                # no run of equal bytes anywhere: zeros / 0xff never blend in
    g.check("untouched")
    g.view[:] = 0                                                      # the payload is the callee's to write
    g.check("payload written")
    g.refill()
    assert np.array_equal(g.view, pattern(1000, start=g.start))


@pytest.mark.parametrize("align,offset", [(16, 0), (16, 4), (16, 8), (256, 0), (256, 12)])
def test_offset_moves_the_payload_off_its_alignment(align, offset):
    g = guarded(64, align=align, offset=offset)
    assert g.ptr % align == offset
    g.check()


def test_one_stray_byte_just_before_the_payload():
    g = guarded(4096)
    g.buf[g.start - 1] ^= 0x01
    _fails_at(g, -1, -1, 1)


def test_one_stray_byte_just_after_the_payload():
    g = guarded(4096)
    g.buf[g.start + 4096] ^= 0x80
    _fails_at(g, 4096, 4096, 1)


def test_one_stray_byte_at_either_far_end():
    g = guarded(4096)
    g.buf[-1] ^= 0xff
    last = g.buf.size - 1 - g.start
    assert last >= 4096 + GUARD - 1
    _fails_at(g, last, last, 1)
    g.refill()
    g.check()
    g.buf[0] ^= 0xff
    _fails_at(g, -g.start, -g.start, 1)


def test_one_stray_byte_in_inter_row_padding():
    h, row_bytes, stride = 5, 40, 104
    g = guarded(h * stride, rows=(h, row_bytes, stride))
    g.view.reshape(h, stride)[:, :row_bytes] = 0                        # every texel written
    g.check("rows written")
    assert (rows_of(g) == 0).all() and rows_of(g, np.uint16).shape == (h, row_bytes // 2)
    g.view[3 * stride + row_bytes] = 0                                 # first padding byte behind row 3
    _fails_at(g, 3 * stride + row_bytes, 3 * stride + row_bytes, 1)
    g.refill()
    g.view[h * stride - 1] ^= 0x10                                     # last padding byte of the last row
    _fails_at(g, h * stride - 1, h * stride - 1, 1)


def test_guards_of_a_strided_surface_hold_four_rows():
    stride = 40000
    g = guarded(2 * stride, rows=(2, 16, stride))
    assert g.start >= 4 * stride and g.buf.size - g.start - 2 * stride >= 4 * stride


def test_a_stray_run_of_zeros():
    g = guarded(4096)
    g.buf[g.start + 4096 + 48:g.start + 4096 + 64] = 0                  # a 16-byte block three blocks past the end
    _fails_at(g, 4096 + 48, 4096 + 63, 16)                            # no pattern byte in that run is 0: every byte counts
    g.refill()
    g.buf[g.start - 8:g.start] = 0xff
    _fails_at(g, -8, -1, 8)


def test_a_changed_source_byte():
    src = np.arange(6 * 7 * 4, dtype=np.uint8).reshape(6, 7, 4)
    for pad in (0, 48):
        f = frozen(src, row_pad=pad)
        assert f.stride == 28 + pad and f.view.shape == src.shape and f.view.strides == (28 + pad, 4, 1)
        assert np.array_equal(f.view, src) and f.view.ctypes.data == f.ptr
        f.check("untouched")
        f.view[2, 3, 1] ^= 0x04
        at = 2 * f.stride + 3 * 4 + 1
        _fails_at(f, at, at, 1)
        f.view[2, 3, 1] ^= 0x04
        f.check("restored")
        f.buf[f.start + 6 * f.stride] ^= 1                             # just behind the source
        _fails_at(f, 6 * f.stride, 6 * f.stride, 1)
    f = frozen(src, row_pad=48)
    f.buf[f.start + 28] ^= 1                                           # padding behind row 0
    _fails_at(f, 28, 28, 1)


def test_frozen_keeps_wider_element_types_and_flat_streams():
    half = (np.arange(3 * 5 * 4, dtype=np.uint16) * 1021).reshape(3, 5, 4)
    f = frozen(half, row_pad=24)
    assert f.view.dtype == np.uint16 and f.stride == 64 and np.array_equal(f.view, half)
    f.view[1, 0, 0] += 1
    _fails_at(f, 64, 64, 1)
    blocks = np.arange(160, dtype=np.uint8)
    f = frozen(blocks)
    assert f.view.shape == (160,) and np.array_equal(f.view, blocks)
    f.check()
    f.view[159] = 0
    _fails_at(f, 159, 159, 1)
