"""Sparse surfaces for the tests that form device and host addresses gigabytes past a surface's base pointer
(tests/test_gpu_large_offsets.py, tests/test_guarded_helper.py).

A surface touches only its rows.  With a row stride of hundreds of MiB, eight short rows span more than 4 GiB of addresses while a few KiB
of them are ever read or written: the 2^31 and 2^32 crossings of every address expression run with images small enough for the CPU
references.  One arena -- a device tensor, or host memory whose untouched pages are never committed -- holds all surfaces of a test, each at
its own `column` (the offset of its first byte), all rows `S` bytes apart:

    arena offset of row r, byte b of a surface = column + r * S + b            S = (span // (h - 1)) & ~15

fence() puts the position-dependent pattern of _guarded.py into the 4 KiB in front of and behind every row, clipped where another
surface's row lies, check_fence() finds any of those bytes changed: a store that missed its row by a few bytes or a few blocks lands there.
(A store whose offset lost its upper bits lands far away; that one is found by the row it did not write -- blank() the target first.)"""
import numpy as np

from _guarded import GuardError, pattern

SPAN_4G = 0x1_5000_0000          # 5.25 GiB: with h = 8, S = 0x30000000; rows 0-2 start below 2^31, rows 3-5 in [2^31, 2^32), rows 6-7 above 2^32
SWITCH_BELOW = (1 << 28) - 16    # h = 8: h * S = 2^31 - 128, the last surface of the 32-bit offset walk (csrc/offset32_host.hpp)
SWITCH_AT = 1 << 28              # h = 8: h * S = 2^31 exactly, the first surface on the 64-bit loaders
FENCE = 4096
ARENA_LIMIT = 6 << 30

_arenas = {}                     # base address -> _Arena


def _is_tensor(x):
    return hasattr(x, "data_ptr")


def _address(x):
    return x.data_ptr() if _is_tensor(x) else x.ctypes.data


class _Surface:
    def __init__(self, column, h, row_bytes, stride):
        self.column, self.h, self.row_bytes, self.stride = column, h, row_bytes, stride

    def rows(self):
        """[(first, end)] arena offsets of the rows"""
        return [(self.column + r * self.stride, self.column + r * self.stride + self.row_bytes) for r in range(self.h)]


class _Arena:
    def __init__(self, buf, whole):
        self.buf, self.whole, self.surfaces = buf, whole, {}


def stride_for(h, span):
    """The row stride of an h-row surface whose last row starts `span` bytes (less up to 16 * (h - 1)) past its first."""
    assert h >= 2 and span >= 16 * (h - 1)
    return (span // (h - 1)) & ~15


def crossings(h, stride):
    """(rows that start below 2^31, in [2^31, 2^32), at or above 2^32) of an h-row surface, as three lists of row numbers"""
    at = [r * stride for r in range(h)]
    return ([r for r in range(h) if at[r] < 1 << 31], [r for r in range(h) if 1 << 31 <= at[r] < 1 << 32], [r for r in range(h) if at[r] >= 1 << 32])


def arena(device, nbytes):
    """One uint8 allocation of `nbytes` bytes at a 256-byte aligned address: torch.empty on `device`, np.empty on the host when device is
    None.  Nothing is written: the host pages stay uncommitted until a row touches them.  release() it when the module is done."""
    assert 0 < nbytes <= ARENA_LIMIT, nbytes
    if device is None:
        whole = np.empty(nbytes + 256, dtype=np.uint8)
    else:
        import torch
        whole = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
    lead = (-_address(whole)) % 256
    buf = whole[lead:lead + nbytes]
    assert _address(buf) % 256 == 0
    _arenas[_address(buf)] = _Arena(buf, whole)
    return buf


def release(buf):
    """Forget the arena and its surfaces.  The caller drops its own reference (`del`), and for a device arena empties torch's cache."""
    _arenas.pop(_address(buf), None)


def reset(buf):
    """Forget the surfaces of the arena: the next test lays out its own."""
    _arenas[_address(buf)].surfaces.clear()


def _find(view):
    ptr = _address(view)
    for a in _arenas.values():
        s = a.surfaces.get(ptr)
        if s is not None:
            return a, s
    raise KeyError("not a sparse() view of a live arena")


def sparse(buf, h, w, texel_bytes, span, column=0, dtype=np.uint8, stride=None):
    """An (h, w, 4) view of the arena `buf` whose rows are S = stride_for(h, span) bytes apart (or `stride`, for the two strides around
    the switch) and whose first byte is the arena's byte `column`.  dtype: the element type, a quarter of a texel (torch: the tensor type
    of that numpy dtype, int16 for uint16).  Surfaces of one test share the arena at columns 64 KiB apart or more."""
    a = _arenas[_address(buf)]
    isz = np.dtype(dtype).itemsize
    assert texel_bytes == 4 * isz, (texel_bytes, dtype)
    S = stride_for(h, span) if stride is None else int(stride)
    row_bytes = w * texel_bytes
    size = buf.numel() if _is_tensor(buf) else buf.size
    assert 0 < S < 1 << 31 and S % isz == 0 and column % isz == 0 and column >= 0, (S, column)
    assert S >= row_bytes, "rows overlap"
    assert (h - 1) * S + row_bytes + column <= size, ("the surface ends behind the arena", h, S, row_bytes, column, size)
    if span >= 1 << 32 and stride is None:
        assert (h - 1) * S >= 1 << 32, ("the last row has to start at or beyond 2^32", h, hex(S))
    s = _Surface(column, h, row_bytes, S)
    mine = s.rows()
    for other in a.surfaces.values():
        for lo, hi in other.rows():
            assert all(hi <= f or e <= lo for f, e in mine), "surfaces overlap"
    if _is_tensor(buf):
        import torch
        tdtype = torch.int16 if np.dtype(dtype) == np.uint16 else torch.from_numpy(np.empty(0, dtype=dtype)).dtype
        flat = buf[:size - size % isz].view(tdtype)
        view = torch.as_strided(flat, (h, w, 4), (S // isz, 4, 1), column // isz)
    else:
        view = np.ndarray(shape=(h, w, 4), dtype=dtype, buffer=buf, offset=column, strides=(S, texel_bytes, isz))
    assert _address(view) == _address(buf) + column
    a.surfaces[_address(view)] = s
    return view


def row_stride(view):
    """bytes between the rows of a sparse() view"""
    return _find(view)[1].stride


def _bytes_of(array):
    return np.ascontiguousarray(array).view(np.uint8).reshape(array.shape[0], -1)


def put(view, array):
    """The texels of `array` (h, w, 4; any dtype of the view's element size) into the rows of the view; nothing else is touched."""
    a, s = _find(view)
    rows = _bytes_of(np.asarray(array))
    assert rows.shape == (s.h, s.row_bytes), (rows.shape, s.h, s.row_bytes)
    if _is_tensor(view):
        import torch
        same_size = {1: np.uint8, 2: np.int16, 4: np.float32}[view.element_size()]
        view.copy_(torch.from_numpy(rows.copy().view(same_size).reshape(tuple(view.shape))).view(view.dtype))
    else:
        view.view(np.uint8)[...] = rows.reshape(s.h, view.shape[1], -1)


def get(view, dtype=None):
    """The rows of the view as a tight numpy array (h, w, 4) of `dtype` (default: the view's own)."""
    a, s = _find(view)
    if _is_tensor(view):
        host = view.cpu().numpy()                      # copies h * w texels, not the span
    else:
        host = np.array(view)
    return host if dtype is None else host.view(dtype)


def _windows(a, s):
    """[(first, end)] arena offsets of the fence bytes of surface `s`: up to FENCE bytes on either side of every row, without the bytes
    of any surface's rows and clipped to the arena"""
    size = a.buf.numel() if _is_tensor(a.buf) else a.buf.size
    taken = sorted(iv for o in a.surfaces.values() for iv in o.rows())
    out = []
    for first, end in s.rows():
        lo, hi = max(0, first - FENCE), min(size, end + FENCE)
        for tf, te in taken:                           # clipped to the nearest row of any surface on either side
            if te <= first:
                lo = max(lo, te)
            if tf >= end:
                hi = min(hi, tf)
        out += [(a_, b_) for a_, b_ in ((lo, first), (end, hi)) if a_ < b_]
    return out


def fence_windows(view):
    """The fence of a view as [(first, end)] arena offsets (for the helper's own tests)."""
    return _windows(*_find(view))


def fence(view):
    """Fill the fence of the view -- FENCE bytes in front of and behind every row, clipped to the neighbouring surfaces' rows -- with the
    _guarded pattern of their arena offsets."""
    a, s = _find(view)
    for lo, hi in _windows(a, s):
        fill = pattern(hi - lo, start=lo)
        if _is_tensor(a.buf):
            import torch
            a.buf[lo:hi].copy_(torch.from_numpy(fill))
        else:
            a.buf[lo:hi] = fill


def blank(view):
    """fence(), and the rows themselves filled with the pattern too: a target whose rows a call has to write, so that a row that was not
    written never looks like one that was (it may hold an earlier test's result)."""
    a, s = _find(view)
    fence(view)
    for lo, hi in s.rows():
        fill = pattern(hi - lo, start=lo)
        if _is_tensor(a.buf):
            import torch
            a.buf[lo:hi].copy_(torch.from_numpy(fill))
        else:
            a.buf[lo:hi] = fill


def check_fence(view, what=""):
    """Raises _guarded.GuardError when a fence byte of the view no longer holds the pattern.  Offsets in the message are relative to the
    view's first byte.  Reads back the windows only."""
    a, s = _find(view)
    bad_first = bad_last = None
    count = 0
    detail = ""
    for lo, hi in _windows(a, s):
        got = a.buf[lo:hi].cpu().numpy() if _is_tensor(a.buf) else np.asarray(a.buf[lo:hi])
        want = pattern(hi - lo, start=lo)
        bad = np.flatnonzero(got != want)
        if bad.size:
            i = int(bad[0])
            if bad_first is None:
                bad_first = lo + i - s.column
                detail = f"first: got {got[i:i + 16].tobytes().hex()} want {want[i:i + 16].tobytes().hex()} (row stride {hex(s.stride)}, {s.h} rows of {s.row_bytes} bytes)"
            bad_last = lo + int(bad[-1]) - s.column
            count += int(bad.size)
    if count:
        raise GuardError(what, bad_first, bad_last, count, detail)
