"""Scenarios for tests/test_gpu_call_combiner.py: N host-pointer CompressBlocks* calls made at the same moment by N host threads, held into
ONE batch of the call combiner (csrc/abi.hip coalesce_small_call) by the hook itwTestCombinerHold, with the combiner's counters read before
and after (itwTestCombinerCounters).  All calls go through the hooks build, a second instance of the library whose combiner is its own.

A request is (format, settings, source pointer, width, height, stride, destination).  Its expected bytes are the CPU oracle's encoding of
that request ALONE -- its own texels under its own settings -- computed before the threads start.  All destinations of a scenario lie in
one guarded allocation (tests/_guarded.py); after the run the whole payload must equal the pattern with every request's bytes in place,
so a block written to another request's place, into a gap or behind the last destination is reported, and so is a missing one."""
import ctypes as C
import threading

import numpy as np

import _dxtex_snorm
from _guarded import guarded

N = 8
HOLD_TIMEOUT_MS = 5000
ENTRY = {"bc1": "CompressBlocksBC1", "bc3": "CompressBlocksBC3", "bc4": "CompressBlocksBC4", "bc5": "CompressBlocksBC5",
         "bc4_snorm": "CompressBlocksBC4S", "bc5_snorm": "CompressBlocksBC5S", "bc7": "CompressBlocksBC7", "bc6h": "CompressBlocksBC6H"}
BPB = {"bc1": 8, "bc3": 16, "bc7": 16, "bc6h": 16, "bc4": 8, "bc5": 16, "bc4_snorm": 8, "bc5_snorm": 16}
KEEPS_PARTIAL = ("bc4", "bc5", "bc4_snorm", "bc5_snorm")
COUNTERS = ("bursts", "batches", "requests", "calls", "hold_timeouts")

_oracle_cache = {}


def texel_bytes(fmt):
    return 8 if fmt == "bc6h" else 4


def want_bytes(oracle, fmt, settings, tex):
    """The oracle's encoding of the texels one request covers: tex (h, w, 4) uint8 / uint16 half bits (bc6h) / int8 (signed formats).
    The ISPC formats drop partial blocks; settings: a Bc7Settings / Bc6hSettings of the binding, or None."""
    tex = np.ascontiguousarray(tex)
    h, w = tex.shape[:2]
    if fmt not in KEEPS_PARTIAL:
        tex = np.ascontiguousarray(tex[:h // 4 * 4, :w // 4 * 4])
    key = (fmt, bytes(settings) if settings is not None else b"", tex.shape, tex.tobytes())
    if key not in _oracle_cache:
        if fmt in ("bc4_snorm", "bc5_snorm"):
            out = _dxtex_snorm.encode(1 if fmt == "bc4_snorm" else 2, tex)
        elif fmt in ("bc4", "bc5"):
            out = oracle.encode_bc45(fmt, tex)
        elif fmt == "bc7":
            out = oracle.encode("bc7", tex, oracle.Bc7Settings.from_buffer_copy(bytes(settings)))
        elif fmt == "bc6h":
            out = oracle.encode("bc6h", tex, oracle.Bc6hSettings.from_buffer_copy(bytes(settings)))
        else:
            out = oracle.encode(fmt, tex)
        _oracle_cache[key] = np.ascontiguousarray(out, dtype=np.uint8).reshape(-1).copy()
    return _oracle_cache[key]


class Source:
    """An image embedded in a byte buffer: rows `stride` bytes apart (row bytes + row_pad), the padding filled with 0x5a."""

    def __init__(self, img, row_pad=0):
        self.img = np.ascontiguousarray(img)
        h = self.img.shape[0]
        row = self.img.shape[1] * 4 * self.img.itemsize
        self.stride = row + row_pad
        self.buf = np.full(h * self.stride + 64, 0x5a, dtype=np.uint8)
        self.buf[:h * self.stride].reshape(h, self.stride)[:, :row] = self.img.view(np.uint8).reshape(h, row)
        self.frozen = self.buf.copy()
        self.ptr = self.buf.ctypes.data

    def unchanged(self):
        return np.array_equal(self.buf, self.frozen)


class RawSource:
    """A byte buffer the test laid out itself (bands of several strides); it must come back unchanged like any source."""

    def __init__(self, buf):
        assert buf.dtype == np.uint8 and buf.flags["C_CONTIGUOUS"]
        self.buf = buf
        self.frozen = buf.copy()
        self.ptr = buf.ctypes.data

    unchanged = Source.unchanged


class Request:
    def __init__(self, fmt, settings, ptr, width, height, stride, dst_off, want):
        self.fmt, self.settings, self.ptr, self.width, self.height, self.stride = fmt, settings, ptr, width, height, stride
        self.dst_off, self.want = dst_off, want


class Scenario:
    """Requests in the order they are given to the threads; destinations consecutive unless `dst` says otherwise."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.reqs = []
        self.sources = []
        self.cursor = 0

    def source(self, img, row_pad=0):
        s = Source(img, row_pad)
        self.sources.append(s)
        return s

    def raw(self, buf):
        s = RawSource(buf)
        self.sources.append(s)
        return s

    def add_raw(self, fmt, settings, ptr, width, height, stride, tex, dst=None, want=None):
        """One request; tex: the texels it covers, in the order the encoder reads them (its oracle input)."""
        if want is None:
            want = want_bytes(self.oracle, fmt, settings, tex)
        off = self.cursor if dst is None else dst
        self.reqs.append(Request(fmt, settings, ptr, width, height, stride, off, want))
        self.cursor = off + want.size
        return self.reqs[-1]

    def add(self, fmt, settings, src, y0, h, x0=0, w=None, dst=None, want=None):
        """Rows y0 .. y0 + h - 1, columns x0 .. x0 + w - 1 of an embedded image, at the image's stride."""
        w = src.img.shape[1] - x0 if w is None else w
        px = 4 * src.img.itemsize
        tex = src.img[y0:y0 + h, x0:x0 + w]
        if fmt in ("bc4_snorm", "bc5_snorm"):
            tex = tex.view(np.int8)
        return self.add_raw(fmt, settings, src.ptr + y0 * src.stride + x0 * px, w, h, src.stride, tex, dst, want)


def counters(T):
    out = (C.c_int64 * 5)()
    T.itwTestCombinerCounters(out)
    return np.array(list(out), dtype=np.int64)


def run(itw, T, sc, hold=None, extra=None):
    """Arm the hold, release one thread per request (plus `extra`, a callable run by one more thread) from a barrier, join, and check
    the bytes: every destination, the gaps between them, the guards around them, the sources.  Returns the counters' deltas as a dict."""
    reqs = sc.reqs
    n = len(reqs)
    assert 1 <= n <= 16
    total = max(r.dst_off + r.want.size for r in reqs) + 4096            # (4096: a gap behind the last destination, inside the payload)
    g = guarded(total)
    expect = g.host().copy()
    claimed = np.zeros(total, dtype=bool)
    for r in reqs:
        assert not claimed[r.dst_off:r.dst_off + r.want.size].any(), "the scenario's destinations overlap"
        claimed[r.dst_off:r.dst_off + r.want.size] = True
        expect[r.dst_off:r.dst_off + r.want.size] = r.want

    calls = []
    for r in reqs:
        surf = itw.RgbaSurface(r.ptr, r.width, r.height, r.stride)
        args = [C.byref(surf), C.c_void_p(g.ptr + r.dst_off)]
        if r.fmt in ("bc7", "bc6h"):
            args.append(C.byref(r.settings))
        calls.append((getattr(T, ENTRY[r.fmt]), args, surf))
    errors = [b"thread did not run"] * n
    barrier = threading.Barrier(n + (1 if extra else 0))
    last_error = T.itwLastError

    def work(i):
        fn, args, _ = calls[i]
        barrier.wait()
        fn(*args)                                # (ctypes drops the GIL for the call)
        errors[i] = last_error()                 # the message is the calling thread's

    def work_extra():
        barrier.wait()
        extra()

    threads = [threading.Thread(target=work, args=(i,)) for i in range(n)]
    if extra:
        threads.append(threading.Thread(target=work_extra))
    before = counters(T)
    T.itwTestCombinerHold(n if hold is None else hold, HOLD_TIMEOUT_MS)
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    after = counters(T)

    assert errors == [None] * n, errors
    got = g.host()
    for i, r in enumerate(reqs):
        mine = got[r.dst_off:r.dst_off + r.want.size]
        if not np.array_equal(mine, r.want):
            bpb = BPB[r.fmt]
            bad = np.flatnonzero((mine.reshape(-1, bpb) != r.want.reshape(-1, bpb)).any(axis=1))
            raise AssertionError(f"request {i} ({r.fmt}, {r.width} x {r.height}, stride {r.stride}): {bad.size}/{r.want.size // bpb} blocks differ from "
                                 f"the oracle's encoding of that request alone; first #{int(bad[0])}")
    stray = np.flatnonzero(got != expect)
    assert stray.size == 0, f"{stray.size} byte(s) outside every destination changed, payload offsets {int(stray[0])} .. {int(stray[-1])}"
    g.check("call combiner scenario")
    for s in sc.sources:
        assert s.unchanged(), "a source was written to"
    return dict(zip(COUNTERS, (int(v) for v in after - before)))
