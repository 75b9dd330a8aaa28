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


# ---- tests/_sparse.py: the arithmetic of the sparse surfaces, on a small host arena ------------------------------------------------------

def test_sparse_stride_rule_and_the_crossings_of_each_span():
    import _sparse as sp
    assert sp.SPAN_4G == 0x150000000 and sp.stride_for(8, sp.SPAN_4G) == 0x30000000
    assert sp.crossings(8, 0x30000000) == ([0, 1, 2], [3, 4, 5], [6, 7])
    assert sp.stride_for(7, sp.SPAN_4G) == 0x38000000 and sp.crossings(7, 0x38000000) == ([0, 1, 2], [3, 4], [5, 6])
    for h in (4, 5, 7, 8, 10, 16, 17, 21, 37, 64):                      # other heights: another stride, the same crossings
        S = sp.stride_for(h, sp.SPAN_4G)
        assert S % 16 == 0 and S < 1 << 31 and sp.SPAN_4G - 16 * (h - 1) <= (h - 1) * S <= sp.SPAN_4G
        low, mid, high = sp.crossings(h, S)
        assert low and mid and high and low + mid + high == list(range(h)) and (h - 1) * S >= 1 << 32
    assert sp.stride_for(3, sp.SPAN_4G) >= 1 << 31                     # three rows or fewer cannot span it with an int32 stride
    # the switch pair: eight rows end 128 bytes below 2^31, and at 2^31
    assert 8 * sp.SWITCH_BELOW == (1 << 31) - 128 and 8 * sp.SWITCH_AT == 1 << 31
    assert sp.crossings(8, sp.SWITCH_BELOW) == (list(range(8)), [], []) and 7 * sp.SWITCH_BELOW + 4112 < 1 << 31


def test_sparse_views_sit_where_the_arithmetic_says_and_move_only_their_rows():
    import _sparse as sp
    A = sp.arena(None, 1 << 20)
    try:
        assert A.ctypes.data % 256 == 0 and A.size == 1 << 20
        A[:] = 0xEE
        span = 7 * 0x12340
        v = sp.sparse(A, 8, 5, 4, span, column=4096)
        S = sp.row_stride(v)
        assert S == 0x12340 and v.shape == (8, 5, 4) and v.strides == (S, 4, 1) and v.ctypes.data == A.ctypes.data + 4096
        u = sp.sparse(A, 8, 3, 8, span, column=4096 + 65536, dtype=np.uint16)
        assert u.strides == (S, 8, 2) and u.dtype == np.uint16
        img = np.arange(8 * 5 * 4, dtype=np.uint8).reshape(8, 5, 4)
        half = (np.arange(8 * 3 * 4, dtype=np.uint16) * 601).reshape(8, 3, 4)
        sp.put(v, img)
        sp.put(u, half)
        assert np.array_equal(sp.get(v), img) and np.array_equal(sp.get(u), half) and sp.get(v).flags["C_CONTIGUOUS"]
        for r in range(8):
            assert np.array_equal(A[4096 + r * S:4096 + r * S + 20], img[r].reshape(-1))
            assert np.array_equal(A[4096 + 65536 + r * S:4096 + 65536 + r * S + 24].view(np.uint16), half[r].reshape(-1))
        touched = np.flatnonzero(A != 0xEE)
        assert touched.size <= 8 * (20 + 24)                           # put() wrote the rows and nothing else
        with pytest.raises(AssertionError):
            sp.sparse(A, 8, 5, 4, span, column=4096 + 8)               # overlaps v
        with pytest.raises(AssertionError):
            sp.sparse(A, 8, 5, 4, span, column=(1 << 20) - 7 * S - 16)  # ends behind the arena
        with pytest.raises(AssertionError):
            sp.sparse(A, 3, 5, 4, 1 << 32, column=0)                   # a stride of 2^31 is no int32
        sp.reset(A)
        with pytest.raises(KeyError):
            sp.get(v)
    finally:
        sp.release(A)


def test_sparse_refuses_a_4g_span_whose_last_row_stays_below_2_32():
    import _sparse as sp
    big = sp.arena(None, sp.ARENA_LIMIT)                               # address space only: no page is touched
    try:
        v = sp.sparse(big, 8, 4, 4, sp.SPAN_4G, column=1 << 16)
        assert sp.row_stride(v) == 0x30000000 and v.ctypes.data == big.ctypes.data + (1 << 16)
        with pytest.raises(AssertionError):
            sp.sparse(big, 60, 4, 4, 1 << 32, column=1 << 20)          # (2^32 // 59) & ~15 times 59 is below 2^32
        with pytest.raises(AssertionError):
            sp.sparse(big, 8, 4, 4, sp.SPAN_4G, column=(6 << 30) - sp.SPAN_4G)     # the last row would end 16 bytes behind the arena
        last = sp.sparse(big, 8, 4, 4, sp.SPAN_4G, column=(6 << 30) - sp.SPAN_4G - 16)
        sp.put(last, np.full((8, 4, 4), 7, np.uint8))                  # touches eight pages of 6 GiB
        assert (sp.get(last) == 7).all() and big[-1] == 7
    finally:
        sp.release(big)


def test_sparse_fence_offsets_and_what_the_fence_catches():
    import _sparse as sp
    A = sp.arena(None, 1 << 20)
    try:
        S = 0x10000
        a = sp.sparse(A, 4, 100, 4, 3 * S, column=8192)                # rows of 400 bytes at 8192 + r * S
        b = sp.sparse(A, 4, 16, 4, 3 * S, column=8192 + 400 + 1000)    # a neighbour 1000 bytes behind a's rows
        c = sp.sparse(A, 4, 16, 4, 3 * S, column=1000)                 # its front fence is clipped by the arena's start
        wa = sp.fence_windows(a)
        assert wa[0] == (8192 - 4096, 8192) and wa[1] == (8592, 9592)  # front: 4 KiB; back: up to b's row
        assert wa[2] == (8192 + S - 4096, 8192 + S) and len(wa) == 8
        assert sp.fence_windows(b)[0] == (8592, 9592) and sp.fence_windows(b)[1] == (9592 + 64, 9592 + 64 + 4096)
        assert sp.fence_windows(c)[0] == (0, 1000) and sp.fence_windows(c)[1] == (1064, 1064 + 4096)
        for v in (a, b, c):
            sp.blank(v)
        for lo, hi in wa:
            assert np.array_equal(A[lo:hi], pattern(hi - lo, start=lo))
        assert np.array_equal(sp.get(a)[1].reshape(-1), pattern(400, start=8192 + S))     # blank(): the rows hold the pattern too
        sp.put(a, np.zeros((4, 100, 4), np.uint8))
        for v in (a, b, c):
            sp.check_fence(v, "rows written")
        A[8192 + 2 * S + 400] ^= 1                                     # the byte behind row 2 of a
        with pytest.raises(GuardError) as e:
            sp.check_fence(a, "helper")
        assert (e.value.first, e.value.last, e.value.count) == (2 * S + 400, 2 * S + 400, 1)
        sp.check_fence(c, "another surface's fence")
        with pytest.raises(GuardError):
            sp.check_fence(b, "shared window")                         # the same byte is in front of b's row 2
        A[8192 + 2 * S + 400] ^= 1
        A[8192 + 3 * S - 16:8192 + 3 * S] = 0                          # a 16-byte block in front of a's row 3
        with pytest.raises(GuardError) as e:
            sp.check_fence(a, "helper")
        assert (e.value.first, e.value.last, e.value.count) == (3 * S - 16, 3 * S - 1, 16)
    finally:
        sp.release(A)
