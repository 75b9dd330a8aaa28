"""Guard bands for the tests that check WHERE an entry point writes (tests/test_gpu_write_extents.py, tests/test_guarded_helper.py).

One allocation `[front guard | payload | back guard]`, all of it -- the payload too -- pre-filled with a position-dependent pattern:
byte i of the allocation = (i * 167 + 13) & 0xff.  An output that was not written therefore never looks like one that was written
correctly, and a stray store lands in memory the test owns: it is reported by an assertion, never by a fault.  Zeros, 0xff and encoded
blocks all differ from the pattern: 167 is odd, so 256 consecutive pattern bytes are 256 different values and no two neighbours are
equal; a stray 8- / 16-byte block equals the 8 / 16 pattern bytes under it with probability 2^-64 / 2^-128 (one specific byte string).

Each guard is at least 64 KiB (a 256-block workgroup tail of 16-byte blocks is 4 KiB) and, for a row-strided surface, at least four
full rows (a decode workgroup can stray by several rows)."""
import numpy as np

GUARD = 65536
_TABLE = ((np.arange(256, dtype=np.uint32) * 167 + 13) & 0xff).astype(np.uint8)


def pattern(n, start=0):
    """Bytes start .. start + n - 1 of the fill pattern (the pattern has period 256)."""
    reps = (n + 255) // 256 + 1
    return np.tile(np.roll(_TABLE, -(start & 255)), reps)[:n].copy()


class GuardError(AssertionError):
    """A byte that had to stay as it was has changed.  first / last: offsets of the first and last changed byte relative to the start
    of the payload (negative: front guard); count: number of changed bytes."""

    def __init__(self, what, first, last, count, detail):
        super().__init__(f"{what}: {count} byte(s) changed that must not, payload offsets {first} .. {last}; {detail}")
        self.first, self.last, self.count = first, last, count


def _is_tensor(x):
    return hasattr(x, "data_ptr")


class _Region:
    """The allocation, the payload's place in it, and which bytes have to survive a call."""

    def __init__(self, nbytes, device, lead, align, offset, rows):
        assert nbytes >= 0 and lead >= 0 and align >= 1 and offset >= 0
        if rows is not None:
            height, row_bytes, stride = rows
            assert stride >= row_bytes and height >= 1 and nbytes == height * stride, (rows, nbytes)
            lead = max(lead, 4 * stride)
        self.rows = rows
        self.nbytes = int(nbytes)
        self.device = device
        total = 2 * lead + align + offset + self.nbytes
        if device is None:
            self.buf = np.empty(total, dtype=np.uint8)
            base = self.buf.ctypes.data
        else:
            import torch
            self.buf = torch.empty(total, dtype=torch.uint8, device=device)
            base = self.buf.data_ptr()
        self.start = lead + (-(base + lead)) % align + offset          # (payload address - offset) is a multiple of `align`
        assert total - self.start - self.nbytes >= lead
        self.ptr = base + self.start
        self.view = self.buf[self.start:self.start + self.nbytes]
        self._expect = pattern(total)
        self._keep = np.ones(total, dtype=bool)                          # bytes that must still equal _expect after a call
        self.refill()

    def refill(self):
        """The whole allocation back to what it held at first: what a second call finds must not be the first call's bytes."""
        if self.device is None:
            self.buf[:] = self._expect
        else:
            import torch
            self.buf.copy_(torch.from_numpy(self._expect))
            if self.buf.is_cuda:
                torch.cuda.synchronize(self.buf.device)

    def _payload_is_free(self):
        s = self.start
        if self.rows is None:
            self._keep[s:s + self.nbytes] = False
        else:
            height, row_bytes, stride = self.rows
            self._keep[s:s + self.nbytes].reshape(height, stride)[:, :row_bytes] = False    # the inter-row padding stays kept

    def _whole(self):
        return self.buf if self.device is None else self.buf.cpu().numpy()

    def host(self):
        """The payload as a numpy array (a copy for a device buffer)."""
        return self._whole()[self.start:self.start + self.nbytes]

    def check(self, what=""):
        got = self._whole()
        bad = np.flatnonzero((got != self._expect) & self._keep)
        if bad.size:
            i = int(bad[0])
            raise GuardError(what, i - self.start, int(bad[-1]) - self.start, int(bad.size),
                             f"first: got {got[i:i + 16].tobytes().hex()} want {self._expect[i:i + 16].tobytes().hex()} "
                             f"(payload: {self.nbytes} bytes" + (f", rows {self.rows}" if self.rows else "") + ")")


def guarded(nbytes, device=None, lead=GUARD, align=16, offset=0, rows=None):
    """An OUTPUT of `nbytes` bytes between two guards.  device None: numpy, else a torch.uint8 tensor on that device.
    .view: the payload (contiguous slice of the same kind), .ptr: its address, .check(what): both guards still hold the pattern bit
    for bit -- and with rows = (height, row_bytes, stride), nbytes = height * stride, so does the padding behind each row; raises
    GuardError otherwise.  .refill() re-patterns everything, .host() is the payload as numpy.
    The payload starts `offset` bytes past a multiple of `align`; each guard has at least `lead` bytes (and four rows)."""
    r = _Region(nbytes, device, lead, align, offset, rows)
    r._payload_is_free()
    return r


def rows_of(g, dtype=np.uint8):
    """The rows of a row-strided guarded(): numpy (height, row_bytes / itemsize) of `dtype`, copied from the payload."""
    height, row_bytes, stride = g.rows
    return np.ascontiguousarray(g.host().reshape(height, stride)[:, :row_bytes]).view(dtype)


def frozen(src, row_pad=0, device=None, lead=GUARD, align=16, offset=0):
    """A SOURCE embedded in a guarded allocation of the same kind (numpy array -> numpy, CUDA tensor -> tensor on its device; a numpy
    array with `device` is uploaded).  row_pad > 0 puts that many pattern bytes behind each row (first axis) of an array of two or more
    axes.  .view: the embedded array / tensor, same shape and dtype, .ptr, .stride (bytes between rows); .check(what): the source AND
    everything around it are unchanged -- every entry point takes its sources as const."""
    if _is_tensor(src):
        device = src.device
        host = src.cpu().numpy()
    else:
        host = np.asarray(src)
    host = np.ascontiguousarray(host)
    isz = host.itemsize
    if host.ndim >= 2:
        height, row_bytes = host.shape[0], int(np.prod(host.shape[1:])) * isz
    else:
        assert row_pad == 0
        height, row_bytes = 1, host.size * isz
    stride = row_bytes + row_pad
    assert stride % isz == 0 and align % isz == 0 and offset % isz == 0
    r = _Region(height * stride, device, lead, align, offset, (height, row_bytes, stride))
    s = r.start
    r._expect[s:s + r.nbytes].reshape(height, stride)[:, :row_bytes] = host.view(np.uint8).reshape(height, row_bytes)
    r.refill()
    r.stride = stride
    inner = [int(np.prod(host.shape[k + 1:])) for k in range(1, host.ndim)]           # element strides of the axes behind the first
    if device is None:
        strides = ((stride,) + tuple(v * isz for v in inner)) if host.ndim >= 2 else (isz,)
        r.view = np.ndarray(shape=host.shape, dtype=host.dtype, buffer=r.buf, offset=s, strides=strides)
    else:
        import torch
        tdtype = torch.from_numpy(np.empty(0, dtype=host.dtype)).dtype if host.dtype != np.uint16 else torch.int16
        flat = r.buf[s:s + r.nbytes].view(tdtype)
        strides = ((stride // isz,) + tuple(inner)) if host.ndim >= 2 else (1,)
        r.view = torch.as_strided(flat, tuple(host.shape), strides)
    return r
