"""The case table and the sequences of tests/test_gpu_stream_order.py; tests/test_stream_order_cases.py checks the table against the
library's exported symbols.  Not a test module: tests import it.  Nothing here needs a GPU until a case is run.

The method.  The caller's stream S is kept busy by a DELAY -- a chain of dependent torch.mm calls of a fixed 4096 x 4096 matrix, its
length calibrated once with event timing -- and the producer of the library call's input is queued behind it.  `ev_ready`, recorded on S
right behind the producer, is the WITNESS: it is read immediately before the library call and must not have fired, or nothing was tested
(the test then fails, it does not skip).  Whatever the library then does on streams of its own has to order itself behind S, and what the
caller queues on S after the call has to come behind the library's work: four sequences (A, B/C, D, E below) check that against references
that never come from the library -- the CPU oracle, the numpy models of tests/_*.py, the from-spec decoders.

  A  device -> device, asynchronous   delay, src <- B, record, witness, CALL, snap = out.clone(), out <- 0xEE, src <- C, synchronise
                                      snap is the reference of B byte for byte (the call read B, the clone saw the call's output); out is
                                      0xEE everywhere (no write of the call came after its place in S); the references of A, B and C
                                      differ in every unit (checked on the CPU), so snap holds nothing of A (read too early) or C (a band
                                      still reading when the caller overwrote the source: one-sided, it can miss, it never fails falsely).
                                      Calls the headers name capturable must also return with the witness still unfired.
  B  device source, synchronous       delay, src <- B, record, witness, CALL; the result is the reference of B and the witness has fired on
  C  ... into host memory             return; a host result is compared before the test synchronises anything.
  D  host source, device target       out holds OLD; delay, snap = out.clone(), record, witness, CALL, synchronise; snap is OLD everywhere
                                      (the call did not overwrite what a reader queued on S had yet to read) and out is the reference.
  E  the shared workspace             two side streams, see the tests.
"""
import ctypes as C
import math
import os
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE, POST, OLD = 0xCD, 0xEE, 0x5A
TARGET_MS = 100.0                                                 # D: see the docstring of tests/test_gpu_stream_order.py

_cache = {}


def cached(key, make):
    if key not in _cache:
        v = make()
        for a in (v if isinstance(v, (list, tuple)) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


# ---- the delay and the report -----------------------------------------------------------------------------------------------------------

class Delay:
    """delay(stream): `reps` dependent torch.mm of a fixed matrix on `stream`, about `target_ms` long (calibrated once, after a warm-up)."""
    N = 4096

    def __init__(self, torch, gpu, target_ms=TARGET_MS):
        self.torch, self.target_ms = torch, target_ms
        g = torch.Generator().manual_seed(1)
        m = torch.eye(self.N) * 0.5 + torch.rand(self.N, self.N, generator=g) / self.N      # row sums about 1: the powers stay finite
        self.m = m.to(gpu)
        self.x = [self.m.clone(), torch.empty_like(self.m)]
        self.own = torch.cuda.Stream(gpu)
        self._timed(4)                                            # the GEMM picks its kernel, the clocks rise
        per = self._timed(16) / 16
        self.reps = max(1, math.ceil(target_ms / per))
        got = self._timed(self.reps)
        if got < target_ms:
            self.reps = math.ceil(self.reps * target_ms / got * 1.1)
            got = self._timed(self.reps)
        self.measured_ms = got

    def _run(self, reps):
        a, b = self.x
        for _ in range(reps):
            self.torch.mm(a, self.m, out=b)
            a, b = b, a

    def _timed(self, reps):
        torch = self.torch
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(self.own):
            t0.record()
            self._run(reps)
            t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    def __call__(self, stream):
        with self.torch.cuda.stream(stream):
            self._run(self.reps)


class Report:
    """What the module measures for its docstring: host milliseconds from ev_ready.record() to the witness and to the return of a call that
    did not wait, and which calls returned before the delay ended."""

    def __init__(self):
        self.max_witness_ms = 0.0
        self.max_return_ms = 0.0
        self.worst = None
        self.early = {}
        self.host_source = {}

    def add(self, name, witness_ms, return_ms=0.0, early=None):
        """early: whether a sequence A call returned with the witness unfired (None: a synchronous call, which has to wait)"""
        self.max_witness_ms = max(self.max_witness_ms, witness_ms)
        if early and return_ms > self.max_return_ms:
            self.max_return_ms, self.worst = return_ms, name
        if early is not None:
            self.early[name] = bool(early)

    def lines(self, delay):
        out = [f"delay: {delay.reps} x mm({delay.N}) = {delay.measured_ms:.1f} ms (target {delay.target_ms:.0f} ms)",
               f"largest host time record -> witness {self.max_witness_ms:.3f} ms, record -> return of a call that did not wait "
               f"{self.max_return_ms:.3f} ms ({self.worst})"]
        out += [f"returned {'before' if e else 'after'} the delay ended: {n}" for n, e in sorted(self.early.items())]
        out += [f"host source, returned {'after' if w else 'before'} the delay ended: {n}" for n, w in sorted(self.host_source.items())]
        return out


class Env:
    def __init__(self, itw, oracle, gpu, torch, delay, stream, report):
        self.itw, self.oracle, self.gpu, self.torch, self.delay, self.S, self.report = itw, oracle, gpu, torch, delay, stream, report

    def dev(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(np.array(a.view(np.int16) if a.dtype == np.uint16 else a)).to(self.gpu)

    def use_stream(self, L=None):
        (L or self.itw.lib()).itwSetStream(self.torch.cuda.current_stream(self.gpu).cuda_stream)


def host_bytes(t):
    a = t.contiguous().cpu().numpy() if hasattr(t, "data_ptr") else np.ascontiguousarray(t)
    return a.view(np.uint8).reshape(-1)


NOT_ARMED = "the delay ended before the call: nothing was tested"


# ---- comparing ----------------------------------------------------------------------------------------------------------------------------

def same_bytes(got, want, what):
    """got: list of uint8 arrays; want: list of arrays of any dtype"""
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        w = np.ascontiguousarray(w).view(np.uint8).reshape(-1)
        assert g.size == w.size, (what, i, g.size, w.size)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, f"output {i}: {bad.size} of {w.size} bytes differ, first at {int(bad[0])}: got {int(g[bad[0]])} want {int(w[bad[0]])}")


def differ_in_every_unit(a, b, units, what):
    """a, b: lists of arrays; units: bytes per unit of each (0: the whole array is one unit; None: an output that need not differ)"""
    for i, (x, y, u) in enumerate(zip(a, b, units)):
        if u is None:
            continue
        x = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        y = np.ascontiguousarray(y).view(np.uint8).reshape(-1)
        assert x.size == y.size and x.size % (u or x.size) == 0, (what, i, x.size, y.size, u)
        d = (x.reshape(-1, u or x.size) != y.reshape(-1, u or x.size)).any(axis=1)
        assert d.all(), (what, f"output {i}: {int((~d).sum())} of {d.size} units of {u} bytes are the same for two contents")


class DeviceCase:
    """Sequence A.  contents[k]: the inputs (numpy arrays) of content k = A, B, C; wants[k]: the reference outputs; units: bytes per
    unit of each output in which the three references differ; call(srcs, outs): the library call on device tensors -- srcs shaped and
    typed as the contents, outs flat uint8 of the wants' sizes (in_place: outs are srcs)."""
    in_place = False
    same = staticmethod(same_bytes)
    differ = staticmethod(differ_in_every_unit)

    def __init__(self, contents, wants, units, call, **kw):
        self.contents, self.wants, self.units, self.call = contents, wants, units, call
        self.before = self.after = None
        self.__dict__.update(kw)


def run_device(name, case, env, must_return_early):
    torch, S = env.torch, env.S
    for k in (0, 2):
        case.differ(case.wants[1], case.wants[k], case.units, (name, "references of B and " + "A C"[k]))
    resident = [[env.dev(a) for a in c] for c in case.contents]
    srcs = [t.clone() for t in resident[0]]
    sizes = getattr(case, "out_sizes", None) or [np.ascontiguousarray(w).nbytes for w in case.wants[1]]
    outs = srcs if case.in_place else [torch.empty(n, dtype=torch.uint8, device=env.gpu) for n in sizes]

    def sequence(timed):
        for s, a in zip(srcs, resident[0]):
            s.copy_(a)
        if not case.in_place:
            for o in outs:
                o.fill_(PRE)
        torch.cuda.synchronize()
        if timed and case.before:
            case.before()
        with torch.cuda.stream(S):
            if timed:
                env.delay(S)
            for s, b in zip(srcs, resident[1]):
                s.copy_(b, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(S)
            t0 = time.perf_counter()
            armed = not ev.query()
            t1 = time.perf_counter()
            case.call(srcs, outs)
            t2 = time.perf_counter()
            early = not ev.query()
            snaps = [o.clone() for o in outs]
            if not case.in_place:
                for o in outs:
                    o.fill_(POST)
            for s, c in zip(srcs, resident[2]):
                s.copy_(c, non_blocking=True)
            S.synchronize()
        return armed, early, snaps, (t1 - t0) * 1e3, (t2 - t0) * 1e3

    sequence(False)                                               # the warm-up: workspace, tables and the allocator's blocks are in place
    torch.cuda.synchronize()
    armed, early, snaps, witness_ms, return_ms = sequence(True)
    torch.cuda.synchronize()
    assert env.itw.last_error() is None, (name, env.itw.last_error())
    assert armed, (name, NOT_ARMED)
    env.report.add(name, witness_ms, return_ms, early)
    case.same([host_bytes(s) for s in snaps], case.wants[1], (name, "what the caller's next kernel on the stream saw"))
    if case.in_place:
        same_bytes([host_bytes(s) for s in srcs], case.contents[2], (name, "the buffers after the caller's last copy"))
    else:
        for i, o in enumerate(outs):
            h = host_bytes(o)
            assert (h == POST).all(), (name, f"output {i}: {int((h != POST).sum())} bytes were written behind the caller's fill")
        same_bytes([host_bytes(s) for s in srcs], case.contents[2], (name, "the sources after the caller's last copy"))
    if case.after:
        case.after()
    if must_return_early:
        assert early, (name, "the call waited for the caller's stream, although its header calls it asynchronous and capturable")


class SyncCase:
    """Sequences B and C.  contents[k]: the inputs of content k = A (warm-up), B; want: the reference outputs of B; call(srcs) -> list of
    results, host arrays or device tensors; host results are compared before anything is synchronised."""
    def __init__(self, contents, want, call, **kw):
        self.contents, self.want, self.call = contents, want, call
        self.__dict__.update(kw)


def run_sync(name, case, env):
    torch, S = env.torch, env.S
    resident = [[env.dev(a) for a in c] for c in case.contents]
    srcs = [t.clone() for t in resident[0]]
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        case.call(srcs)                                           # the warm-up, on content A
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        env.delay(S)
        for s, b in zip(srcs, resident[1]):
            s.copy_(b, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(S)
        t0 = time.perf_counter()
        armed = not ev.query()
        t1 = time.perf_counter()
        res = case.call(srcs)
        waited = ev.query()
        check = getattr(case, "check", None)
        if not check:
            for i, r in enumerate(res):
                if not hasattr(r, "data_ptr"):                    # host memory: compared before the test synchronises anything
                    same_bytes([host_bytes(r)], [case.want[i]], (name, f"host result {i} on return"))
        S.synchronize()
    torch.cuda.synchronize()
    assert env.itw.last_error() is None, (name, env.itw.last_error())
    assert armed, (name, NOT_ARMED)
    env.report.add(name, (t1 - t0) * 1e3)
    if check:
        check(res, (name, "the results"))
    else:
        same_bytes([host_bytes(r) for r in res], case.want, (name, "the results"))
    assert waited, (name, "a synchronous call returned while its device source was still being produced on the caller's stream")


class HostSourceCase:
    """Sequence D.  call(out): host texels into the device tensor `out` (flat uint8 of want's size)."""

    def __init__(self, want, call):
        self.want, self.call = want, call


def run_host_source(name, case, env):
    torch, S = env.torch, env.S
    out = torch.empty(case.want.size, dtype=torch.uint8, device=env.gpu)
    with torch.cuda.stream(S):
        case.call(out)                                            # the warm-up
    out.fill_(OLD)
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        env.delay(S)
        snap = out.clone()
        ev = torch.cuda.Event()
        ev.record(S)
        t0 = time.perf_counter()
        armed = not ev.query()
        t1 = time.perf_counter()
        case.call(out)
        waited = ev.query()
        S.synchronize()
    torch.cuda.synchronize()
    assert env.itw.last_error() is None, (name, env.itw.last_error())
    assert armed, (name, NOT_ARMED)
    env.report.add(name, (t1 - t0) * 1e3)
    env.report.host_source[name] = bool(waited)                  # (reported, not asserted: the bytes below are the check)
    h = host_bytes(snap)
    assert (h == OLD).all(), (name, f"{int((h != OLD).sum())} of {h.size} bytes of the destination were overwritten before a reader "
                                    "queued on the caller's stream ahead of the call had read them")
    same_bytes([host_bytes(out)], [case.want], (name, "the destination"))


# ---- content and references --------------------------------------------------------------------------------------------------------------

BPB = {"bc1": 8, "bc3": 16, "bc4": 8, "bc5": 16, "bc4_snorm": 8, "bc5_snorm": 16, "bc6h": 16, "bc7": 16, "etc1": 8}
ENTRY = {"bc1": "CompressBlocksBC1", "bc3": "CompressBlocksBC3", "bc4": "CompressBlocksBC4", "bc5": "CompressBlocksBC5", "bc4_snorm": "CompressBlocksBC4S",
         "bc5_snorm": "CompressBlocksBC5S", "bc6h": "CompressBlocksBC6H", "bc7": "CompressBlocksBC7", "etc1": "itwCompressBlocksETC1"}


def texels(fmt, prof, w, h, k):
    """Content k of a format: itw_amd.surfaces with a seed of its own; the BC7 alpha profiles get an opaque right half."""
    def make():
        from itw_amd import surfaces
        seed = surfaces.SEED + 400 + 17 * k
        if fmt == "bc6h":
            return surfaces.hdr_smooth(h, w, seed=seed)
        if fmt in ("bc4_snorm", "bc5_snorm"):
            return surfaces.snorm_normal_map(h, w, seed=seed, strength=3.0 + k)
        img = surfaces.ldr_smooth(h, w, seed=seed).copy()
        if (prof or "").startswith("alpha"):
            img[:, w // 2:, 3] = 255
        return img
    return cached(("texels", fmt, (prof or "").startswith("alpha"), w, h, k), make)


def encoded(env, fmt, prof, img, key):
    """The reference stream of `img`: the CPU oracle; DirectXTex's own encoder for the signed formats; the reference library for ETC1."""
    def make():
        if fmt in ("bc4", "bc5"):
            return env.oracle.encode_bc45(fmt, img)
        if fmt in ("bc4_snorm", "bc5_snorm"):
            import _dxtex_snorm
            return _dxtex_snorm.encode(1 if fmt == "bc4_snorm" else 2, img).reshape(-1)
        if fmt == "etc1":
            import _etc1
            _etc1.live_reference()
            return _etc1.ref_encode(img, 6)                       # the `slow` profile
        return env.oracle.encode_mt(fmt, img, prof).reshape(-1)
    return cached(("encoded", fmt, prof, key), make)


def settings_of(itw, fmt, prof):
    return itw.bc7_profile(prof) if fmt == "bc7" else itw.bc6h_profile(prof) if fmt == "bc6h" else itw.etc_profile("slow") if fmt == "etc1" else None


def blocks_call(L, itw, fmt, ptr, w, h, stride, dst, settings):
    """CompressBlocks* of library instance L with raw pointers"""
    surf = itw.RgbaSurface(ptr, w, h, stride)
    fn = getattr(L, ENTRY[fmt])
    if settings is None:
        fn(C.byref(surf), C.c_void_p(dst))
    else:
        fn(C.byref(surf), C.c_void_p(dst), C.byref(settings))


def route_counters(itw):
    T = itw.test_lib()
    buf = (C.c_int64 * len(itw.BC7_ROUTE_COUNTERS))()
    T.itwTestBc7RouteCounters(buf, len(buf))
    return dict(zip(itw.BC7_ROUTE_COUNTERS, list(buf)))


# ---- A: the builders ----------------------------------------------------------------------------------------------------------------------

def a_blocks(fmt, prof=None, w=64, h=64, path=None, hooks=False, routes=None):
    """CompressBlocks* device -> device.  path: itwSetBc7Path for the call; hooks: through the hooks build, `routes` the counters the timed
    call must leave (name -> count)."""
    def build(env):
        itw = env.itw
        L = itw.test_lib() if hooks else itw.lib()
        contents = [[texels(fmt, prof, w, h, k)] for k in range(3)]
        wants = [[encoded(env, fmt, prof, c[0], (w, h, k))] for k, c in enumerate(contents)]
        st = settings_of(itw, fmt, prof)
        es = 2 if fmt == "bc6h" else 1

        def call(srcs, outs):
            env.use_stream(L)
            if path:
                L.itwSetBc7Path(itw.abi.BC7_PATH[path])
            try:
                blocks_call(L, itw, fmt, srcs[0].data_ptr(), w, h, srcs[0].stride(0) * es, outs[0].data_ptr(), st)
            finally:
                if path:
                    L.itwSetBc7Path(0)
            assert L.itwLastError() is None, L.itwLastError()

        case = DeviceCase(contents, wants, [BPB[fmt]], call)
        if routes is not None:
            case.before = itw.test_lib().itwTestBc7RouteCountersReset

            def after():
                got = route_counters(itw)
                assert {n: got[n] for n in routes} == routes, (fmt, prof, w, h, got)
            case.after = after
        return case
    return build


def _noise8(h, w, k, seed):
    """uint8 texels of content k: A, B and C live in disjoint thirds of the code range, so that whatever averages them differs too"""
    rng = np.random.default_rng(seed * 3 + k)
    return rng.integers(8 + 85 * k, 8 + 85 * k + 70, (h, w, 4), dtype=np.uint8)


def _normal8(h, w, k, seed):
    """uint8 normal-map texels (tests/test_gpu_normal_bc5.py's content: zero vectors, axis vectors and extreme codes among noise)"""
    from test_gpu_normal_bc5 import _content
    return cached(("normal8", h, w, k, seed), lambda: _content(h, w, seed * 3 + k))


def a_normal_bc5(w=64, h=64, ops=7):
    def build(env):
        import _normal_prep as N
        contents = [[_normal8(h, w, k, 500)] for k in range(3)]
        wants = [[cached(("normal bc5", w, h, k, ops), lambda: env.oracle.encode_bc45("bc5", np.ascontiguousarray(N.prepare_rgba8(c[0], ops))))]
                 for k, c in enumerate(contents)]
        return DeviceCase(contents, wants, [16], lambda srcs, outs: env.itw.compress_normal_map(srcs[0], ops=ops, out=outs[0]))
    return build


def a_normal_bc5s(kind, w=64, h=64, ops=7):
    def build(env):
        import _dxtex_snorm as D
        import _normal_snorm as S
        contents = [[S.content(kind, h, w, 510 + k)] for k in range(3)]
        wants = [[cached(("normal bc5s", kind, w, h, k, ops), lambda: D.encode(2, np.ascontiguousarray(S.quantize(c[0], ops))).reshape(-1))]
                 for k, c in enumerate(contents)]
        return DeviceCase(contents, wants, [16], lambda srcs, outs: env.itw.compress_normal_map_snorm(srcs[0], ops=ops, out=outs[0]))
    return build


def a_prepare_normal(half, sizes=((64, 64), (12, 20)), ops=7):
    """itwPrepareNormalMapChain, in place: the sources are the outputs"""
    def build(env):
        import _normal_prep as N
        import _mipgen as M

        def content(h, w, k):
            return M.seeded_half_image(h, w, 520 + k) if half else _normal8(h, w, k, 521)
        contents = [[content(h, w, k) for h, w in sizes] for k in range(3)]
        wants = [[np.ascontiguousarray(N.prepare(a, ops)) for a in c] for c in contents]
        return DeviceCase(contents, wants, [a.shape[1] * a.itemsize * 4 for a in contents[0]],
                          lambda srcs, outs: env.itw.prepare_normal_map(srcs, ops=ops), in_place=True)
    return build


def _as_image(t, torch, shape, es):
    """a flat uint8 tensor as an (h, w, 4) image of element size es"""
    return (t.view(torch.int16) if es == 2 else t.view(torch.int8) if es == -1 else t).view(*shape)


def a_quantize_normal(kind, sizes=((64, 64), (12, 20)), ops=7):
    def build(env):
        import _normal_snorm as S
        contents = [[S.content(kind, h, w, 530 + k) for h, w in sizes] for k in range(3)]
        wants = [[np.ascontiguousarray(S.quantize(a, ops)) for a in c] for c in contents]

        def call(srcs, outs):
            env.itw.quantize_normal_map(srcs, ops=ops, out=[_as_image(o, env.torch, s.shape, -1) for o, s in zip(outs, srcs)])
        return DeviceCase(contents, wants, [w * 4 for h, w in sizes], call)
    return build


def a_pad(w, h, pixel_size):
    def build(env):
        def content(k):
            rng = np.random.default_rng(540 + k)
            return rng.integers(0, 256, (h, w, 4), dtype=np.uint8) if pixel_size == 4 else rng.integers(0, 65536, (h, w, 4), dtype=np.uint16)
        W, H = (w + 3) & ~3, (h + 3) & ~3
        contents = [[content(k)] for k in range(3)]
        wants = [[np.pad(c[0], ((0, H - h), (0, W - w), (0, 0)), mode="edge")] for c in contents]

        def call(srcs, outs):
            env.use_stream()
            surf = env.itw.RgbaSurface(srcs[0].data_ptr(), w, h, srcs[0].stride(0) * srcs[0].element_size())
            env.itw.lib().itwPadToMultipleOf4Device(C.byref(surf), pixel_size, C.c_void_p(outs[0].data_ptr()))
        return DeviceCase(contents, wants, [W * pixel_size], call)
    return build


def a_convert(to16, w=203, h=3, depth=32, planes=4, alpha=1):
    def build(env):
        from test_prepass_convert import _oracle8, _oracle16, _source
        contents = [[np.ascontiguousarray(_source(np.random.default_rng(550 + k), depth, planes, w, h))] for k in range(3)]
        wants = [[_oracle16(env.oracle, c[0], depth, planes, alpha, w, h) if to16 else _oracle8(env.oracle, c[0], depth, planes, alpha, 1, w, h)] for c in contents]
        L = env.itw.lib()

        def call(srcs, outs):
            env.use_stream()
            if to16:
                rc = L.itwConvertToRGBA16FDevice(C.c_void_p(srcs[0].data_ptr()), depth, planes, alpha, w, h, C.c_void_p(outs[0].data_ptr()))
            else:
                rc = L.itwConvertToRGBA8Device(C.c_void_p(srcs[0].data_ptr()), depth, planes, alpha, 1, w, h, C.c_void_p(outs[0].data_ptr()))
            assert rc == 0
        # (the model plants the same six special values at the head of every content: a row is the unit)
        return DeviceCase(contents, wants, [w * (8 if to16 else 4)], call)
    return build


def _stream_of(env, fmt, sizes, k):
    """(blocks, [texels], modes) of a random stream for images of `sizes`, decoded by the from-spec decoders (tests/test_gpu_decode_chain.py)"""
    from test_gpu_decode_chain import _case
    return _case(env.itw, env.oracle, fmt, list(sizes), seed=560 + k)


def a_decode(fmt, entry, sizes):
    """entry: 'blocks' (itwDecodeBlocks, one image of whole blocks), 'image' (itwDecodeImage, any size) or 'chain' (itwDecodeChain)"""
    def build(env):
        itw, torch = env.itw, env.torch
        cases = [_stream_of(env, fmt, sizes, k) for k in range(3)]
        contents = [[np.array(c[0])] for c in cases]
        wants = [list(c[1]) + [c[2]] for c in cases]              # the texels of every image, then the modes of the whole stream
        es = 2 if fmt == "bc6h" else 1

        def call(srcs, outs):
            imgs = [_as_image(o, torch, (h, w, 4), es) for o, (h, w) in zip(outs, sizes)]
            modes = outs[-1].view(torch.int32)
            env.use_stream()
            if entry == "blocks":
                (h, w), = sizes
                rc = itw.lib().itwDecodeBlocks(itw.DXGI_FORMAT[fmt], C.c_void_p(srcs[0].data_ptr()), w, h, C.c_void_p(imgs[0].data_ptr()), w * 4 * es,
                                               C.c_void_p(modes.data_ptr()))
            elif entry == "image":
                rc = itw.lib().itwDecodeImage(itw.DXGI_FORMAT[fmt], C.c_void_p(srcs[0].data_ptr()), C.cast(itw.abi._surfaces(imgs), C.c_void_p),
                                              C.c_void_p(modes.data_ptr()), None)
            else:
                rc = itw.lib().itwDecodeChain(itw.DXGI_FORMAT[fmt], C.c_void_p(srcs[0].data_ptr()), C.cast(itw.abi._surfaces(imgs), C.c_void_p), len(imgs),
                                              C.c_void_p(modes.data_ptr()), None)
            assert rc == 0, itw.last_error()
        # random blocks: the reserved BC7 blocks decode alike in every content, so a row of texels is the unit; the modes follow the block
        # index in every content (and are 0 for the formats without modes): compared, not required to differ
        return DeviceCase(contents, wants, [w * 4 * es for h, w in sizes] + [None], call)
    return build


def a_preview(zoom, surface=False, fmt="bc7", w=64, h=64, view_w=48, view_h=40):
    def build(env):
        import _preview
        itw = env.itw
        cases = [_stream_of(env, fmt, [(h, w)], k) for k in range(3)]
        view = dict(view_w=view_w, view_h=view_h, x=3, y=2, zoom=zoom, matte=0x00C86432)
        contents = [[c[1][0] if surface else np.array(c[0])] for c in cases]
        wants = [[_preview.viewport(c[1][0], view_w, view_h, 3, 2, zoom, 4 + 8 + 16, 0x00C86432, 1.0)] for c in cases]

        def call(srcs, outs):
            out = outs[0].view(view_h, view_w, 3)
            if surface:
                itw.preview_surface(srcs[0], out=out, **view)
            else:
                itw.preview(fmt, srcs[0], w, h, out=out, **view)
        return DeviceCase(contents, wants, [view_w * 3], call)
    return build


class _MeasureCase(DeviceCase):
    @staticmethod
    def same(got, want, what):
        from test_gpu_measure import _same
        import itw_amd
        n = C.sizeof(itw_amd.ErrorStats)
        stats, maps = want
        raw = got[0].tobytes()
        assert len(raw) == n * len(stats)
        for i, s in enumerate(stats):
            _same(itw_amd.ErrorStats.from_buffer_copy(raw[i * n:(i + 1) * n]), s, (what, i))
        if len(got) > 1:
            assert np.array_equal(got[1].view(np.uint64).astype(np.int64), maps[0]), (what, "block_sse")

    @staticmethod
    def differ(b, other, units, what):
        for i, (x, y) in enumerate(zip(b[0], other[0])):
            assert x["sse"] != y["sse"] and x["worst_block_sse"] != y["worst_block_sse"], (what, i)
        for x, y in zip(b[1], other[1]):
            assert (x != y).all(), (what, "block_sse")


def a_measure(chain, fmt="bc7", sizes=((64, 64),)):
    """itwMeasureBlocks (stats words and the per-block map) / itwMeasureChain (one stats record per image); all pointers on the device"""
    def build(env):
        from test_gpu_measure import _expect, _random_source
        itw, torch = env.itw, env.torch
        n = C.sizeof(itw.ErrorStats)
        bpb = BPB[fmt]

        def make(k):
            blocks = np.array(_stream_of(env, fmt, sizes, k)[0])
            srcs = [_random_source(fmt, h, w, 570 + 7 * k + i) for i, (h, w) in enumerate(sizes)]
            stats, maps, at = [], [], 0
            for s in srcs:
                nb = ((s.shape[0] + 3) // 4) * ((s.shape[1] + 3) // 4)
                st, bm = _expect(itw, env.oracle, fmt, blocks[at * bpb:(at + nb) * bpb], s)
                stats.append(st)
                maps.append(bm)
                at += nb
            return [blocks] + srcs, (stats, maps)
        made = [cached(("measure", chain, fmt, sizes, k), lambda: make(k)) for k in range(3)]
        contents, wants = [m[0] for m in made], [m[1] for m in made]

        def call(srcs, outs):
            if chain:
                env.use_stream()
                arr = itw.abi._surfaces(srcs[1:])
                rc = itw.lib().itwMeasureChain(C.cast(arr, C.c_void_p), len(sizes), C.c_void_p(srcs[0].data_ptr()), itw.DXGI_FORMAT[fmt], C.c_void_p(outs[0].data_ptr()), n)
                assert rc == 0, itw.last_error()
            else:
                itw.measure_async(fmt, srcs[0], srcs[1], outs[0], outs[1].view(torch.int64))
        case = _MeasureCase(contents, wants, None, call)
        # run_device sizes the outputs from wants[1]: give it arrays of the sizes
        nb0 = ((sizes[0][0] + 3) // 4) * ((sizes[0][1] + 3) // 4)
        case.out_sizes = [n * len(sizes)] + ([] if chain else [nb0 * 8])
        return case
    return build


def _mip_content(kind, h, w, k, alpha_cutout=False):
    def make():
        if kind == "half":
            rng = np.random.default_rng(580 + k)
            return (rng.random((h, w, 4), dtype=np.float32) * np.float32(0.8) + np.float32(0.1 + k)).astype(np.float16).view(np.uint16)
        img = _noise8(h, w, k, 581)
        if alpha_cutout:
            import _alpha_mips as A
            img = img.copy()
            img[..., 3] = A.cutout(h, w, 582 + k, hole=False)[..., 3]
        return img
    return cached(("mip content", kind, h, w, k, alpha_cutout), make)


def a_mips(kind, w=64, h=64, per_level=False, srgb=False, alpha=None):
    """itwGenerateMipChain; alpha = (weight, coverage_ref): itwGenerateMipChainAlpha.  The base is the source, levels 1 .. are the outputs."""
    def build(env):
        import _alpha_mips as A
        import _mipgen as M
        import _srgb_mips as SR
        itw, torch = env.itw, env.torch
        contents = [[_mip_content(kind, h, w, k, alpha is not None)] for k in range(3)]

        def model(base):
            if alpha is not None:
                return A.chain(base, srgb=srgb, weight=alpha[0], ref=alpha[1])[0][1:]
            return (SR.chain(base) if srgb else M.chain(base))[1:]
        wants = [cached(("mips", kind, w, h, srgb, alpha, k), lambda: [np.ascontiguousarray(l) for l in model(c[0])]) for k, c in enumerate(contents)]
        es = 2 if kind == "half" else 1
        shapes = [tuple(l.shape) for l in wants[1]]

        def call(srcs, outs):
            chain = [srcs[0]] + [_as_image(o, torch, s, es) for o, s in zip(outs, shapes)]
            if alpha is not None:
                itw.generate_mips_into([chain], per_level=per_level, srgb=srgb, alpha_weight=alpha[0], alpha_coverage=alpha[1])
            else:
                itw.generate_mips_into([chain], per_level=per_level, srgb=srgb)
        # colour lives in disjoint ranges per content, so every texel of every level differs
        return DeviceCase(contents, wants, [4 * es for s in shapes], call)
    return build


def a_image_mt(fmt="bc1", prof=None, w=64, h=64):
    """CompressImageMT with device pointers on both sides: one CompressBlocks* call on the calling thread (csrc/dispatch.hip), so asynchronous"""
    def build(env):
        itw = env.itw
        contents = [[texels(fmt, prof, w, h, k)] for k in range(3)]
        wants = [[encoded(env, fmt, prof, c[0], (w, h, k))] for k, c in enumerate(contents)]

        def call(srcs, outs):
            env.use_stream()
            surf = itw.RgbaSurface(srcs[0].data_ptr(), w, h, srcs[0].stride(0))
            assert itw.lib().CompressImageMT(C.byref(surf), C.c_void_p(outs[0].data_ptr()), itw.image_func(fmt, prof), itw.DXGI_FORMAT[fmt])
        return DeviceCase(contents, wants, [BPB[fmt]], call)
    return build


# ---- B / C: the builders ------------------------------------------------------------------------------------------------------------------

def b_blocks_to_host(fmt, prof=None, w=64, h=64, mt=None):
    """CompressBlocks* (mt: through 'CompressImageMT' / 'CompressImageST'), device texels into host memory: compress_single_run"""
    def build(env):
        itw = env.itw
        L = itw.lib()
        contents = [[texels(fmt, prof, w, h, k)] for k in range(2)]
        want = [encoded(env, fmt, prof, contents[1][0], (w, h, 1))]
        st = settings_of(itw, fmt, prof)
        es = 2 if fmt == "bc6h" else 1

        def call(srcs):
            out = np.full(want[0].size, PRE, np.uint8)
            env.use_stream()
            if mt:
                surf = itw.RgbaSurface(srcs[0].data_ptr(), w, h, srcs[0].stride(0) * es)
                assert getattr(L, mt)(C.byref(surf), C.c_void_p(out.ctypes.data), itw.image_func(fmt, prof), itw.DXGI_FORMAT[fmt])
            else:
                blocks_call(L, itw, fmt, srcs[0].data_ptr(), w, h, srcs[0].stride(0) * es, out.ctypes.data, st)
            return [out]
        return SyncCase(contents, want, call)
    return build


SLICED = [("bc1", None), ("bc7", "veryfast"), ("bc6h", "fast")]       # the SLICED table of tests/test_gpu_write_extents.py, at its size
SLICED_W, SLICED_H, SLICE_PIXELS = 256, 192, 4096


def _sliced_settings(itw, fmt, prof):
    return settings_of(itw, fmt, prof) or itw.Bc7Settings()      # ignored for the other formats; selects the Ex entry point


def _window_of_two(itw, call):
    itw.lib().itwSetSliceWindow(2)
    try:
        return call()
    finally:
        itw.lib().itwSetSliceWindow(0)


def b_sliced(fmt, prof, to_host, ex=True):
    """itwCompressImageSlicedEx (ex False: itwCompressImageSliced with the format's trampoline) from device texels: 12 slices in 6 windows"""
    def build(env):
        itw, torch = env.itw, env.torch
        w, h = SLICED_W, SLICED_H
        contents = [[texels(fmt, prof, w, h, k)] for k in range(2)]
        want = [encoded(env, fmt, prof, contents[1][0], (w, h, 1))]
        st = _sliced_settings(itw, fmt, prof) if ex else None

        def call(srcs):
            out = np.full(want[0].size, PRE, np.uint8) if to_host else torch.full((want[0].size,), PRE, dtype=torch.uint8, device=env.gpu)
            ok, _ = _window_of_two(itw, lambda: itw.compress_image(fmt, srcs[0], prof, slice_pixels=SLICE_PIXELS, out=out, settings=st))
            assert ok
            return [out]
        return SyncCase(contents, want, call)
    return build


def _chain_images(itw, shape, k):
    def make():
        from itw_amd import surfaces
        seed = surfaces.SEED + 600 + 13 * k
        if shape == "mips":                                       # 20 x 12 with its mips: one gathered group
            return itw.mip_chain(surfaces.ldr_smooth(12, 20, seed=seed))
        if shape == "unaligned":
            return [surfaces.ldr_smooth(13, 21, seed=seed)]
        return [surfaces.ldr_smooth(4, 4, seed=seed), surfaces.ldr_smooth(1024, 2048, seed=seed + 1)]       # 131 072 blocks: encoded in place
    return cached(("chain images", shape, k), make)


def _chain_want(env, fmt, prof, shape, k):
    from test_gpu_chain import _oracle_chain
    return cached(("chain want", fmt, prof, shape, k), lambda: _oracle_chain(env.itw, env.oracle, fmt, _chain_images(env.itw, shape, k), prof))


def b_chain(fmt, prof, shape, to_host, own_function=False, normal=None):
    """itwCompressImageChainEx from device images; own_function: itwCompressImageChain with a caller's own CompressionFunc, the literal loop;
    normal 'unorm': itwCompressNormalMapChain (flips and normalise in the gather), 'snorm': itwCompressSignedNormalMapChain (int8 sources)"""
    def build(env):
        itw, torch = env.itw, env.torch
        if normal == "snorm":
            import _dxtex_snorm as D
            import _normal_snorm as S
            contents = [[S.content("int8", h, w, 630 + 3 * k + i) for i, (h, w) in enumerate(((12, 20), (6, 10), (3, 5)))] for k in range(2)]
            want = [cached(("chain snorm", fmt), lambda: np.concatenate([D.encode(2, np.ascontiguousarray(S.quantize(a, 7))).reshape(-1) for a in contents[1]]))]
        elif normal == "unorm":
            import _normal_prep as N
            from test_gpu_chain import _oracle_chain
            contents = [_chain_images(itw, shape, k) for k in range(2)]
            want = [cached(("chain normal", fmt, shape), lambda: _oracle_chain(itw, env.oracle, fmt, [np.ascontiguousarray(N.prepare_rgba8(a, 7)) for a in contents[1]], prof))]
        else:
            contents = [_chain_images(itw, shape, k) for k in range(2)]
            want = [_chain_want(env, fmt, prof, shape, 1)]
        L = itw.lib()
        if own_function:
            assert fmt == "bc1"
            from itw_amd.abi import COMPRESSION_FUNC
            fn = COMPRESSION_FUNC(lambda surf, dst: L.CompressBlocksBC1(surf, dst))

        def call(srcs):
            out = np.full(want[0].size, PRE, np.uint8) if to_host else torch.full((want[0].size,), PRE, dtype=torch.uint8, device=env.gpu)
            if normal == "snorm":
                ok, _ = itw.compress_chain_normal_snorm(fmt, srcs, ops=7, out=out)
            else:
                ok, _ = itw.compress_chain(fmt, srcs, prof, out=out, cmp_func=C.cast(fn, C.c_void_p) if own_function else None,
                                           normal_ops=7 if normal == "unorm" else None)
            assert ok
            return [out]
        return SyncCase(contents, want, call)
    return build


def b_mipped(fmt, prof, to_host, w=64, h=64, srgb=False, alpha=None):
    """itwCompressImageMipped from a device base; srgb: itwCompressImageMippedEx with ITW_MIP_SRGB; alpha = (weight, coverage_ref):
    itwCompressImageMippedAlpha"""
    def build(env):
        import _alpha_mips as A
        import _mipgen as M
        import _srgb_mips as SR
        from test_gpu_chain import _oracle_chain
        itw, torch = env.itw, env.torch
        contents = [[_mip_content("byte", h, w, k, True) if alpha else texels(fmt, prof, w, h, k)] for k in range(2)]

        def model(base):
            return A.chain(base, srgb=srgb, weight=alpha[0], ref=alpha[1])[0] if alpha else SR.chain(base) if srgb else M.chain(base)
        want = [cached(("mipped", fmt, prof, w, h, srgb, alpha), lambda: _oracle_chain(itw, env.oracle, fmt, model(contents[1][0]), prof))]

        def call(srcs):
            out = np.full(want[0].size, PRE, np.uint8) if to_host else torch.full((want[0].size,), PRE, dtype=torch.uint8, device=env.gpu)
            ok, _ = itw.compress_mipped(fmt, srcs[0], profile=prof, out=out, srgb=srgb, alpha_weight=bool(alpha and alpha[0]), alpha_coverage=alpha[1] if alpha else 0)
            assert ok
            return [out]
        return SyncCase(contents, want, call)
    return build


def b_mipped_normal_snorm(to_host, w=64, h=64, ops=7):
    """itwCompressSignedNormalMapMipped from a device base of int8 texels: widen, filter, normalise and quantise, DirectXTex's BC5S"""
    def build(env):
        import _dxtex_snorm as D
        import _mipgen as M
        import _normal_snorm as S
        from test_gpu_normal_snorm_chain import widen_model
        itw, torch = env.itw, env.torch
        contents = [[S.content("int8", h, w, 610 + k)] for k in range(2)]

        def model():
            levels = M.chain(widen_model(contents[1][0], ops))
            return np.concatenate([D.encode(2, np.ascontiguousarray(S.quantize(lv, ops & 4))).reshape(-1) for lv in levels])
        want = [cached(("mipped snorm", w, h, ops), model)]

        def call(srcs):
            out = np.full(want[0].size, PRE, np.uint8) if to_host else torch.full((want[0].size,), PRE, dtype=torch.uint8, device=env.gpu)
            ok, _ = itw.compress_mipped_normal_snorm("bc5_snorm", srcs[0], ops=ops, out=out)
            assert ok
            return [out]
        return SyncCase(contents, want, call)
    return build


def b_alpha_coverage(sizes=((64, 64), (12, 20)), ref=128):
    """itwAlphaCoverage: the counts come back in host memory, so the call has to wait for the images' producer"""
    def build(env):
        contents = [[np.random.default_rng(620 + 5 * k + i).integers(0, 256, (h, w, 4), dtype=np.uint8) for i, (h, w) in enumerate(sizes)] for k in range(2)]
        want = [np.array([int((c[..., 3] >= ref).sum()) for c in contents[1]], np.uint64)]
        assert all(int((a[..., 3] >= ref).sum()) != int(want[0][i]) for i, a in enumerate(contents[0]))
        return SyncCase(contents, want, lambda srcs: [np.array(env.itw.alpha_coverage(srcs, ref), np.uint64)])
    return build


def b_refined(entry, w=64, h=64, fmt="bc7", first="veryfast", refine="slow", mask=7):
    """entry: 'refined' | 'to_a' | 'to_b' | 'chain' | 'chain_to'; every byte and every stat field against the predictions of tests/_refine*.py"""
    def build(env):
        import _refine as R
        import _refine_chain as RC
        import _refine_target as T
        itw, oracle = env.itw, env.oracle
        if entry == "chain_to":
            contents = [_chain_images(itw, "mips", k) for k in range(2)]
            key = ("stream order chain", 1)
            want = RC.predict_to(oracle, fmt, key, contents[1], first, refine, mask, max_listed=8)
            call = lambda srcs: itw.compress_chain_refined_to(fmt, srcs, first, refine, max_listed=8, channels="rgb", want_block_map=True,
                                                              want_tier_map=True, want_image_stats=True)
            same = RC.same_to
        elif entry == "chain":
            contents = [_chain_images(itw, "mips", k) for k in range(2)]
            key = ("stream order chain", 1)
            ea = RC.tier(oracle, fmt, key, contents[1], first, mask)[1]
            want = RC.predict(oracle, fmt, key, contents[1], first, refine, mask, int(np.median(ea)))
            call = lambda srcs: itw.compress_chain_refined(fmt, srcs, first, refine, int(np.median(ea)), channels="rgb", want_block_map=True,
                                                           want_tier_map=True, want_image_stats=True)
            same = RC.same
        else:
            contents = [[texels(fmt, first, w, h, k)] for k in range(2)]
            img, key = contents[1][0], ("stream order", w, h, 1)
            ea = R.tier(oracle, fmt, key, img, first, mask)[1]
            kw = dict(channels="rgb", want_block_map=True, want_tier_map=True)
            if entry == "refined":
                want = R.predict(oracle, fmt, key, img, first, refine, mask, int(np.median(ea)))
                call = lambda srcs: itw.compress_refined(fmt, srcs[0], first, refine, int(np.median(ea)), **kw)
                same = R.same
            elif entry == "to_a":
                want = T.predict(oracle, fmt, key, img, first, refine, mask, max_listed=64)
                call = lambda srcs: itw.compress_refined_to(fmt, srcs[0], first, refine, max_listed=64, **kw)
                same = T.same
            else:
                target = int(ea.sum()) * 9 // 10
                want = T.predict(oracle, fmt, key, img, first, refine, mask, target=target)
                call = lambda srcs: itw.compress_refined_to(fmt, srcs[0], first, refine, target_sse=target, **kw)
                same = T.same
        assert want["listed"] > 0 and want["replaced"] > 0, (entry, want["listed"], want["replaced"])
        return SyncCase(contents, want, call, check=lambda res, what: same(res, want, what))
    return build


# ---- D: the builders ----------------------------------------------------------------------------------------------------------------------

def _knob(name, value, call):
    os.environ[name] = value
    try:
        return call()
    finally:
        del os.environ[name]


def d_blocks(fmt, prof, w=64, h=64, runs=None):
    """CompressBlocks* from host texels into device memory; runs: under ITW_HOST_RUNS, the staged runs (compress_runs)"""
    def build(env):
        itw = env.itw
        img = texels(fmt, prof, w, h, 1)
        want = encoded(env, fmt, prof, img, (w, h, 1))
        st = settings_of(itw, fmt, prof)

        def call(out):
            env.use_stream()
            go = lambda: blocks_call(itw.lib(), itw, fmt, img.ctypes.data, w, h, img.strides[0], out.data_ptr(), st)
            _knob("ITW_HOST_RUNS", runs, go) if runs else go()
        return HostSourceCase(want, call)
    return build


def d_sliced(fmt, prof):
    def build(env):
        itw = env.itw
        img = texels(fmt, prof, SLICED_W, SLICED_H, 1)
        want = encoded(env, fmt, prof, img, (SLICED_W, SLICED_H, 1))
        st = _sliced_settings(itw, fmt, prof)

        def call(out):
            env.use_stream()
            ok, _ = _window_of_two(itw, lambda: itw.compress_image(fmt, img, prof, slice_pixels=SLICE_PIXELS, out=out, settings=st))
            assert ok
        return HostSourceCase(want, call)
    return build


def d_chain(fmt, prof, shape):
    def build(env):
        itw = env.itw
        images = _chain_images(itw, shape, 1)
        want = _chain_want(env, fmt, prof, shape, 1)

        def call(out):
            ok, _ = itw.compress_chain(fmt, images, prof, out=out)
            assert ok
        return HostSourceCase(want, call)
    return build


# ---- the table ----------------------------------------------------------------------------------------------------------------------------

class Case:
    """id; scheme 'A' (run_device), 'B' (run_sync; the host-target ones are the issue's C) or 'D' (run_host_source); the exported symbols the
    case calls; build(env) -> the case object; capturable: the header calls the entry point asynchronous and capturable, so it must return
    before the delay ends."""

    def __init__(self, id, scheme, symbols, build, capturable=False):
        self.id, self.scheme, self.symbols, self.build, self.capturable = id, scheme, tuple(symbols), build, capturable


TWO = {"TWO_BANDS": 1}
CASES = [Case(f"blocks-{f}", "A", [ENTRY[f]], a_blocks(f), True) for f in ("bc1", "bc3", "bc4", "bc5", "bc4_snorm", "bc5_snorm")] + [
    Case("blocks-etc1", "A", ["itwCompressBlocksETC1", "itwGetProfile_etc_slow"], a_blocks("etc1", "slow"), True),
    Case("blocks-bc6h-fast", "A", ["CompressBlocksBC6H", "GetProfile_bc6h_fast"], a_blocks("bc6h", "fast"), True),
    Case("blocks-bc6h-slow", "A", ["CompressBlocksBC6H", "GetProfile_bc6h_slow"], a_blocks("bc6h", "slow"), True),
    Case("blocks-bc7-wide-slow", "A", ["CompressBlocksBC7", "GetProfile_slow", "itwSetBc7Path"], a_blocks("bc7", "slow", path="wide", hooks=True, routes={"WIDE": 1}), True),
    Case("blocks-bc7-wide-alpha_slow", "A", ["CompressBlocksBC7", "GetProfile_alpha_slow", "itwSetBc7Path"],
         a_blocks("bc7", "alpha_slow", path="wide", hooks=True, routes={"WIDE": 1}), True),
    # 512 x 256 = 8192 blocks = 32 chunks of 256: the first size at which two_bands() holds (csrc/bc7.hip); 496 x 256 = 31 chunks is the control.
    # A call of this size takes the wide shape on its own, so the deep one is asked for, as tests/test_gpu_bc7_pairs.py does.
    Case("blocks-bc7-two-bands-slow", "A", ["CompressBlocksBC7"], a_blocks("bc7", "slow", 512, 256, path="deep", hooks=True, routes={"TWO_BANDS": 1, "PILOT": 1, "RGB_BOUNDED": 1}), True),
    Case("blocks-bc7-two-bands-alpha_slow", "A", ["CompressBlocksBC7"],
         a_blocks("bc7", "alpha_slow", 512, 256, path="deep", hooks=True, routes={"TWO_BANDS": 1, "ALPHA_FIRST_BOUNDED7": 1}), True),
    Case("blocks-bc7-one-band-slow", "A", ["CompressBlocksBC7"], a_blocks("bc7", "slow", 496, 256, path="deep", hooks=True, routes={"TWO_BANDS": 0, "PILOT": 0, "RGB_BOUNDED": 1}), True),
    Case("blocks-bc7-one-band-alpha_slow", "A", ["CompressBlocksBC7"],
         a_blocks("bc7", "alpha_slow", 496, 256, path="deep", hooks=True, routes={"TWO_BANDS": 0, "ALPHA_FIRST_BOUNDED7": 1}), True),
    Case("image-mt-device-to-device", "A", ["CompressImageMT", "CompressImageBC1"], a_image_mt()),
    Case("normal-bc5", "A", ["itwCompressNormalMapBC5"], a_normal_bc5(), True),
] + [Case(f"normal-bc5s-{k}", "A", ["itwCompressNormalMapBC5S"], a_normal_bc5s(k), True) for k in ("int8", "half", "float")] + [
    Case("prepare-normal-chain-rgba8", "A", ["itwPrepareNormalMapChain"], a_prepare_normal(False)),
    Case("prepare-normal-chain-rgba16f", "A", ["itwPrepareNormalMapChain"], a_prepare_normal(True)),
] + [Case(f"quantize-normal-chain-{k}", "A", ["itwQuantizeNormalMapChain"], a_quantize_normal(k)) for k in ("half", "float")] + [
    Case("pad-5x7-rgba8", "A", ["itwPadToMultipleOf4Device"], a_pad(5, 7, 4)),
    Case("pad-127x9-rgba16f", "A", ["itwPadToMultipleOf4Device"], a_pad(127, 9, 8)),
    Case("convert-rgba8", "A", ["itwConvertToRGBA8Device"], a_convert(False)),
    Case("convert-rgba16f", "A", ["itwConvertToRGBA16FDevice"], a_convert(True)),
] + [Case(f"decode-blocks-{f}", "A", ["itwDecodeBlocks"], a_decode(f, "blocks", [(64, 64)]), True) for f in ("bc1", "bc7", "bc6h")] + [
    Case("decode-image-bc3-20x12", "A", ["itwDecodeImage"], a_decode("bc3", "image", [(12, 20)]), True),
    Case("decode-chain-bc7", "A", ["itwDecodeChain"], a_decode("bc7", "chain", [(12, 20), (6, 10), (3, 5)])),
    Case("preview-blocks-zoom1", "A", ["itwPreviewBlocks"], a_preview(1.0), True),
    Case("preview-blocks-zoom4", "A", ["itwPreviewBlocks"], a_preview(4.0, w=256, h=192), True),
    Case("preview-surface", "A", ["itwPreviewSurface"], a_preview(1.0, surface=True), True),
    Case("measure-blocks-bc7", "A", ["itwMeasureBlocks"], a_measure(False), True),
    Case("measure-chain-bc7", "A", ["itwMeasureChain"], a_measure(True, sizes=((12, 20), (6, 10), (3, 5)))),
    Case("mips-pyramid-rgba8", "A", ["itwGenerateMipChain"], a_mips("byte")),
    Case("mips-per-level-rgba8", "A", ["itwGenerateMipChain"], a_mips("byte", per_level=True)),
    Case("mips-pyramid-rgba16f", "A", ["itwGenerateMipChain"], a_mips("half")),
    Case("mips-per-level-rgba16f", "A", ["itwGenerateMipChain"], a_mips("half", per_level=True)),
    Case("mips-srgb", "A", ["itwGenerateMipChain"], a_mips("byte", srgb=True)),
    Case("mips-linear-20x12", "A", ["itwGenerateMipChain"], a_mips("byte", 20, 12)),
    Case("mips-alpha-weight-coverage", "A", ["itwGenerateMipChainAlpha"], a_mips("byte", alpha=(True, 128))),
    # B, device -> host (the issue's C: the host array is compared on return)
] + [Case(f"to-host-{f}{'-' + p if p else ''}", "B", [ENTRY[f]], b_blocks_to_host(f, p))
     for f, p in (("bc1", None), ("bc3", None), ("bc4", None), ("bc5", None), ("bc4_snorm", None), ("bc5_snorm", None), ("etc1", "slow"), ("bc6h", "fast"), ("bc7", "basic"))] + [
    Case("image-mt-device-to-host", "B", ["CompressImageMT", "CompressImageBC1"], b_blocks_to_host("bc1", mt="CompressImageMT")),
    Case("image-st-device-to-host", "B", ["CompressImageST", "CompressImageBC3"], b_blocks_to_host("bc3", mt="CompressImageST")),
] + [Case(f"sliced-{f}-to-{'host' if th else 'device'}", "B", ["itwCompressImageSlicedEx", "itwSetSliceWindow"], b_sliced(f, p, th)) for f, p in SLICED for th in (False, True)] + [
    Case("sliced-trampoline-bc7-to-device", "B", ["itwCompressImageSliced", "CompressImageBC7_veryfast"], b_sliced("bc7", "veryfast", False, ex=False)),
] + [
    Case(f"chain-mips-to-{'host' if th else 'device'}", "B", ["itwCompressImageChainEx"], b_chain("bc7", "veryfast", "mips", th)) for th in (False, True)] + [
    Case(f"chain-in-place-to-{'host' if th else 'device'}", "B", ["itwCompressImageChainEx"], b_chain("bc1", None, "in place", th)) for th in (False, True)] + [
    Case(f"chain-own-function-to-{'host' if th else 'device'}", "B", ["itwCompressImageChain", "itwPadToMultipleOf4Device"], b_chain("bc1", None, "unaligned", th, own_function=True))
    for th in (False, True)] + [
    Case("chain-normal-map-bc5", "B", ["itwCompressNormalMapChain"], b_chain("bc5", None, "mips", False, normal="unorm")),
    Case("chain-signed-normal-map-bc5s", "B", ["itwCompressSignedNormalMapChain"], b_chain("bc5_snorm", None, "mips", False, normal="snorm")),
] + [Case(f"mipped-bc1-to-{'host' if th else 'device'}", "B", ["itwCompressImageMipped"], b_mipped("bc1", None, th)) for th in (False, True)] + [
    Case("mipped-srgb-bc1", "B", ["itwCompressImageMippedEx"], b_mipped("bc1", None, False, srgb=True)),
    Case("mipped-alpha-bc3", "B", ["itwCompressImageMippedAlpha"], b_mipped("bc3", None, False, alpha=(True, 128))),
] + [
    Case(f"mipped-normal-snorm-to-{'host' if th else 'device'}", "B", ["itwCompressSignedNormalMapMipped"], b_mipped_normal_snorm(th)) for th in (False, True)] + [
    Case("alpha-coverage", "B", ["itwAlphaCoverage"], b_alpha_coverage()),
    Case("refined", "B", ["itwCompressImageRefined"], b_refined("refined")),
    Case("refined-to-policy-a", "B", ["itwCompressImageRefinedTo"], b_refined("to_a")),
    Case("refined-to-policy-b", "B", ["itwCompressImageRefinedTo"], b_refined("to_b")),
    Case("chain-refined", "B", ["itwCompressImageChainRefined"], b_refined("chain")),
    Case("chain-refined-to", "B", ["itwCompressImageChainRefinedTo"], b_refined("chain_to")),
    # D, host -> device
    Case("host-to-device-bc1", "D", ["CompressBlocksBC1"], d_blocks("bc1", None)),
    Case("host-to-device-bc7-basic", "D", ["CompressBlocksBC7", "GetProfile_basic"], d_blocks("bc7", "basic")),
    Case("host-to-device-runs-bc7", "D", ["CompressBlocksBC7"], d_blocks("bc7", "slow", 64, 256, runs="0.125,0.625")),
    Case("host-to-device-runs-bc6h", "D", ["CompressBlocksBC6H"], d_blocks("bc6h", "fast", 64, 256, runs="0.125,0.625")),
] + [Case(f"host-to-device-sliced-{f}", "D", ["itwCompressImageSlicedEx"], d_sliced(f, p)) for f, p in SLICED] + [
    Case("host-to-device-chain-mips", "D", ["itwCompressImageChainEx"], d_chain("bc7", "veryfast", "mips")),
]
# E, the shared workspace across two streams: tests/test_gpu_stream_order.py::test_e_*
WORKSPACE_SYMBOLS = ("CompressBlocksBC7", "CompressBlocksBC6H", "itwSetStream")

IDS = [c.id for c in CASES]
assert len(set(IDS)) == len(IDS)


def covered_symbols():
    return {s for c in CASES for s in c.symbols} | set(WORKSPACE_SYMBOLS)
