"""Every entry point that takes a row stride, with surfaces whose rows lie more than 2 and more than 4 GiB past their base pointer.

The surfaces are sparse (tests/_sparse.py): a few short rows, hundreds of MiB apart, in one arena that is allocated once for the module.
With eight rows 0x30000000 bytes apart rows 0-2 start below 2^31, rows 3-5 in [2^31, 2^32) and rows 6-7 above 2^32, so an address that went
through an int32 or a uint32 on its way misplaces whole rows: the result then differs from the reference in those rows.  The images are a
few hundred blocks or a few thousand texels, so the expected bytes come from the CPU references of each feature's own test, computed on
the tight image.  Where a feature's reference is a compiled library of fixed availability or a recording of fixed sizes (BC4/BC5_SNORM,
ETC1, BC1A, BC2, BC3_DXTEX, the signed normal sources, the BC6H signed reading, ETC1 / BC2 decode), the expected bytes are those of the same
call on a tight copy of the same texels -- each such test says so.

Every sparse surface is fenced (4 KiB of pattern in front of and behind each row) and checked after the call; sources are read back and
must be unchanged; targets are pre-filled with the pattern, so a row that was not written is seen.

BC1 / BC3 / BC4 / BC5 choose between a 32-bit offset walk and 64-bit loaders (csrc/offset32_host.hpp); they also run at the two strides
around that switch, eight rows 2^28 - 16 and 2^28 bytes apart, and itwTestWalks32 -- the function the launchers branch on -- says which
side each call took."""
import ctypes as C
import functools

import numpy as np
import pytest

import _sparse as sp
from conftest import first_mismatch

pytestmark = pytest.mark.gpu

ARENA_BYTES = sp.SPAN_4G + (64 << 20)        # 5.31 GiB: the span, and 64 MiB of columns
COL = 1 << 16                                # surfaces of one test sit at multiples of 64 KiB
TINY_STRIDE = 0x7FFFFFF0                     # levels of two or three rows cannot span 4 GiB with an int32 stride: the largest one instead
_skipped = []


# ---- the arenas ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def device_arena(gpu):
    import torch
    free = torch.cuda.mem_get_info(gpu)[0]
    if free < ARENA_BYTES + (512 << 20):
        yield None
        return
    buf = sp.arena(gpu, ARENA_BYTES)
    yield buf
    sp.release(buf)
    del buf
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def host_memory():
    buf = sp.arena(None, ARENA_BYTES)            # address space: only the rows' pages are ever touched
    yield buf
    sp.release(buf)
    del buf


@pytest.fixture
def arena(device_arena, request):
    if device_arena is None:
        _skipped.append(request.node.name)
        pytest.skip("less free device memory than the arena needs")
    sp.reset(device_arena)
    return device_arena


@pytest.fixture
def host_arena(host_memory):
    sp.reset(host_memory)
    return host_memory


@pytest.fixture(scope="module", autouse=True)
def _errors_return(itw):
    """a call the library refuses leaves a message and fails an assertion here; the default mode would abort the session"""
    for L in (itw.lib(), itw.test_lib()):
        L.itwSetErrorMode(itw.ON_ERROR_RETURN)
    yield
    for L in (itw.lib(), itw.test_lib()):
        L.itwSetErrorMode(itw.ON_ERROR_ABORT)


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_device_fault(itw, gpu):
    """an address error here can be a fault instead of a wrong byte: then the session ends, nothing more is started on that device"""
    itw.lib().itwClearError()
    yield
    import torch
    assert itw.lib().itwLastError() is None, itw.lib().itwLastError()
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, no further test runs on it: {e}", returncode=3)


# ---- content, placing, checking ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ldr(h, w, seed, dtype="uint8"):
    a = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8).view(dtype)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _hdr(h, w, seed):
    rng = np.random.default_rng(seed)
    a = (rng.random((h, w, 4), dtype=np.float32) * np.float32(6.0) + np.float32(0.05)).astype(np.float16).view(np.uint16)
    a.setflags(write=False)
    return a


def _span_args(h, span):
    """sparse()'s span or stride for an image of h rows: ("stride", S) asks for one; else the 4 GiB span where four rows or more can
    carry it, the largest int32 stride for two or three rows"""
    if isinstance(span, tuple):
        return dict(span=0, stride=span[1])
    if h >= 4:
        return dict(span=sp.SPAN_4G)
    return dict(span=0, stride=TINY_STRIDE if h > 1 else 1 << 20)


def _source(buf, img, column, span=None):
    """`img` as a fenced sparse surface of the arena"""
    h, w = img.shape[:2]
    v = sp.sparse(buf, h, w, 4 * img.itemsize, column=column, dtype=img.dtype, **_span_args(h, span))
    sp.fence(v)
    sp.put(v, img)
    return v


def _target(buf, h, w, dtype, column, span=None):
    """a fenced sparse surface whose rows hold the pattern: every texel has to be written"""
    v = sp.sparse(buf, h, w, 4 * np.dtype(dtype).itemsize, column=column, dtype=dtype, **_span_args(h, span))
    sp.blank(v)
    return v


def _unchanged(v, img, what):
    sp.check_fence(v, f"{what}: source fence")
    assert np.array_equal(sp.get(v, np.uint8), np.ascontiguousarray(img).view(np.uint8)), (what, "the call changed its source")      # (bytes: a NaN stays a NaN)


def _written(v, want, what):
    sp.check_fence(v, f"{what}: target fence")
    got = sp.get(v, want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got.view(np.uint8) != np.ascontiguousarray(want).view(np.uint8)).reshape(got.shape[0], -1).any(axis=1))
    assert bad.size == 0, (what, f"rows {bad.tolist()} of {got.shape[0]} differ (row stride {hex(sp.row_stride(v))}); "
                                 f"row {bad[0]}: got {got[bad[0]].reshape(-1)[:8].tolist()} want {want[bad[0]].reshape(-1)[:8].tolist()}")


def _sync():
    import torch
    torch.cuda.synchronize()


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _dev(gpu, a):
    import torch
    return torch.from_numpy(np.array(a.view(np.int16) if a.dtype == np.uint16 else a)).to(gpu)


def _same_blocks(got, want, bpb, what):
    got, want = _host(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.size == want.size, (what, got.size, want.size)
    m = first_mismatch(got, want, bpb)
    assert m is None, (what, m)


# ---- A. encode, source side ----------------------------------------------------------------------------------------------------------------

_refs = {}


def _cpu_encode(oracle, fmt, prof, img, key):
    k = (fmt, prof, key)
    if k not in _refs:
        r = oracle.encode_bc45(fmt, img) if fmt in ("bc4", "bc5") else oracle.encode_mt(fmt, img, prof)
        r.setflags(write=False)
        _refs[k] = r
    return _refs[k]


def _tight_encode(itw, gpu, fmt, prof, img, key):
    """the same call on a tight copy of the same texels"""
    k = ("tight", fmt, prof, key)
    if k not in _refs:
        r = _host(itw.compress(fmt, _dev(gpu, img), prof))
        _sync()
        _refs[k] = r
    return _refs[k]


def test_the_crossings_of_the_spans_used_here():
    """what every case below relies on (the helper asserts the rest when a surface is laid out)"""
    assert sp.crossings(8, sp.stride_for(8, sp.SPAN_4G)) == ([0, 1, 2], [3, 4, 5], [6, 7])
    assert sp.crossings(7, sp.stride_for(7, sp.SPAN_4G)) == ([0, 1, 2], [3, 4], [5, 6])
    assert sp.crossings(16, sp.stride_for(16, sp.SPAN_4G))[2] == [12, 13, 14, 15]
    assert sp.crossings(3, TINY_STRIDE) == ([0, 1], [2], [])
    assert ARENA_BYTES <= sp.ARENA_LIMIT


BPB = {"bc1": 8, "bc3": 16, "bc4": 8, "bc5": 16, "bc4_snorm": 8, "bc5_snorm": 16, "bc7": 16, "bc6h": 16, "etc1": 8, "bc1a": 8, "bc2": 16,
       "bc3_dxtex": 16}
WHOLE = (8, 1028)                            # 2 block rows of 257 blocks: one lane past a workgroup
PARTIAL = (7, 1025)                          # the same with a tail, for the formats that keep partial blocks
PLAIN = [("bc1", None, WHOLE, "cpu"), ("bc3", None, WHOLE, "cpu"),
         ("bc4", None, PARTIAL, "cpu"), ("bc5", None, PARTIAL, "cpu"), ("bc4", None, WHOLE, "cpu"), ("bc5", None, WHOLE, "cpu"),
         ("bc4_snorm", None, PARTIAL, "tight"), ("bc5_snorm", None, PARTIAL, "tight"),
         ("bc6h", "fast", WHOLE, "cpu"), ("bc6h", "slow", WHOLE, "cpu"),
         ("etc1", "slow", WHOLE, "tight"), ("bc1a", None, PARTIAL, "tight"), ("bc2", None, PARTIAL, "tight"), ("bc3_dxtex", None, PARTIAL, "tight")]


def _texels_for(fmt, size, seed=1):
    h, w = size
    if fmt == "bc6h":
        return _hdr(h, w, seed)
    return _ldr(h, w, seed, "int8" if fmt.endswith("_snorm") else "uint8")


@pytest.mark.parametrize("fmt,prof,size,ref", PLAIN, ids=[f"{f}-{p or '-'}-{s[1]}x{s[0]}" for f, p, s, r in PLAIN])
def test_encode_from_a_source_that_spans_4_gib(itw, gpu, oracle, arena, fmt, prof, size, ref):
    """Expected: the CPU oracle ("cpu"); for BC4/BC5_SNORM, ETC1, BC1A, BC2 and BC3_DXTEX, whose references are compiled from a tree that is
    not always there, the same call on a tight copy of the same texels ("tight")."""
    img = _texels_for(fmt, size)
    want = _cpu_encode(oracle, fmt, prof, img, size) if ref == "cpu" else _tight_encode(itw, gpu, fmt, prof, img, size)
    v = _source(arena, img, 3 * COL)
    assert sp.row_stride(v) * (size[0] - 1) >= 1 << 32
    if fmt in ("bc1", "bc3", "bc4", "bc5", "bc4_snorm", "bc5_snorm"):
        assert itw.test_lib().itwTestWalks32(3 if fmt == "bc3" else 1 if fmt == "bc1" else 4, sp.row_stride(v), size[1], size[0]) == 0
    got = itw.compress(fmt, v, prof)
    _sync()
    _same_blocks(got, want, BPB[fmt], (fmt, prof, size))
    _unchanged(v, img, (fmt, prof))


BC7 = [(p, path) for p in ("veryfast", "slow", "alpha_slow") for path in ("deep", "wide")]


@pytest.mark.parametrize("prof,path", BC7, ids=[f"{p}-{q}" for p, q in BC7])
def test_bc7_from_a_source_that_spans_4_gib(itw, gpu, oracle, arena, prof, path):
    """through the hooks build, whose route counters say which launch shape the call took"""
    import torch
    h, w = WHOLE
    img = _ldr(h, w, 7)
    want = _cpu_encode(oracle, "bc7", prof, img, WHOLE)
    v = _source(arena, img, 5 * COL)
    T = itw.test_lib()
    out = torch.empty(want.size, dtype=torch.uint8, device=gpu)
    names = itw.BC7_ROUTE_COUNTERS
    buf = (C.c_int64 * len(names))()
    T.itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
    T.itwSetBc7Path(itw.abi.BC7_PATH[path])
    try:
        T.itwTestBc7RouteCountersReset()
        st = itw.bc7_profile(prof)
        T.CompressBlocksBC7(C.byref(itw.RgbaSurface(v.data_ptr(), w, h, sp.row_stride(v))), C.c_void_p(out.data_ptr()), C.byref(st))
        _sync()
    finally:
        T.itwSetBc7Path(0)
    assert T.itwLastError() is None, T.itwLastError()
    T.itwTestBc7RouteCounters(buf, len(names))
    route = dict(zip(names, list(buf)))
    branches = names[:8]
    assert sum(route[n] for n in branches) == 1 and route["PROBE_IGNORED"] == 0, route
    assert (route["WIDE"] == 1) == (path == "wide"), (path, route)
    _same_blocks(out, want, 16, (prof, path))
    _unchanged(v, img, (prof, path))


def _normal_img(h, w):
    from test_gpu_normal_bc5 import _content
    return _content(h, w, 77)


def test_bc5_normal_map_ops_7_from_a_source_that_spans_4_gib(itw, gpu, oracle, arena):
    import _normal_prep as N
    h, w = PARTIAL
    img = _normal_img(h, w)
    want = oracle.encode_bc45("bc5", np.ascontiguousarray(N.prepare_rgba8(img, 7)))
    v = _source(arena, img, 2 * COL)
    got = itw.compress_normal_map(v, ops=7)
    _sync()
    _same_blocks(got, want, 16, "bc5 normal ops 7")
    _unchanged(v, img, "bc5 normal")


@pytest.mark.parametrize("kind", ["int8", "half", "float"])
def test_bc5s_signed_normal_sources_that_span_4_gib(itw, gpu, arena, kind):
    """4-, 8- and 16-byte texels.  Expected: the same call on a tight copy of the same texels (the reference encoder is a compiled library)."""
    import _normal_snorm as S
    for size in (PARTIAL, WHOLE):
        h, w = size
        img = S.content(kind, h, w, 31)
        want = _host(itw.compress_normal_map_snorm(S.torch_of(img, gpu), ops=7))
        sp.reset(arena)
        v = _source(arena, img, 4 * COL)
        got = itw.compress_normal_map_snorm(v, ops=7)
        _sync()
        _same_blocks(got, want, 16, ("bc5s normal", kind, size))
        _unchanged(v, img, ("bc5s normal", kind))
        assert itw.test_lib().itwTestWalks32(S.texel_bytes(img), sp.row_stride(v), w, h) == 0


# the switch: eight rows end 128 bytes below 2^31 (32-bit walk, offsets up to 1.75 GiB) and at 2^31 (64-bit loaders); and each again from a
# source 4 bytes past a 16-byte boundary, which takes the dword-load instantiations
SWITCH = [(name, S, walks, off) for name, S, walks in (("below", sp.SWITCH_BELOW, 1), ("at", sp.SWITCH_AT, 0)) for off in (0, 4)]
SWITCH_IDS = [f"{n}-{'aligned' if o == 0 else 'plus4'}" for n, S, k, o in SWITCH]


@pytest.mark.parametrize("name,stride,walks,off", SWITCH, ids=SWITCH_IDS)
@pytest.mark.parametrize("fmt", ["bc1", "bc3", "bc4", "bc5"])
def test_both_sides_of_the_switch_between_the_32_bit_walk_and_the_64_bit_loaders(itw, gpu, oracle, arena, fmt, name, stride, walks, off):
    h, w = WHOLE
    img = _ldr(h, w, 1)
    want = _cpu_encode(oracle, fmt, None, img, WHOLE)
    assert itw.test_lib().itwTestWalks32({"bc1": 1, "bc3": 3}.get(fmt, 4), stride, w, h) == walks
    v = _source(arena, img, 6 * COL + off, span=("stride", stride))
    assert v.data_ptr() % 16 == off and sp.row_stride(v) == stride
    got = itw.compress(fmt, v)
    _sync()
    _same_blocks(got, want, BPB[fmt], (fmt, name, off))
    _unchanged(v, img, (fmt, name, off))


@pytest.mark.parametrize("name,stride,walks,off", SWITCH, ids=SWITCH_IDS)
def test_both_sides_of_the_switch_bc5_normal_maps(itw, gpu, oracle, arena, name, stride, walks, off):
    """itwCompressNormalMapBC5 with ops 7 against the CPU oracle over the prepared texels; itwCompressNormalMapBC5S of every source kind
    against the same call on a tight copy"""
    import _normal_prep as N
    import _normal_snorm as S
    h, w = WHOLE
    img = _normal_img(h, w)
    want = oracle.encode_bc45("bc5", np.ascontiguousarray(N.prepare_rgba8(img, 7)))
    v = _source(arena, img, 6 * COL + off, span=("stride", stride))
    got = itw.compress_normal_map(v, ops=7)
    _sync()
    _same_blocks(got, want, 16, ("bc5 normal", name, off))
    _unchanged(v, img, ("bc5 normal", name, off))
    for i, kind in enumerate(S.KINDS):                             # 4-, 8- and 16-byte texels: each has its own block row in the walk's rule
        src = S.content(kind, h, w, 32)
        assert itw.test_lib().itwTestWalks32(S.texel_bytes(src), stride, w, h) == walks
        want = _host(itw.compress_normal_map_snorm(S.torch_of(src, gpu), ops=7))
        u = _source(arena, src, (9 + 2 * i) * COL + off, span=("stride", stride))
        got = itw.compress_normal_map_snorm(u, ops=7)
        _sync()
        _same_blocks(got, want, 16, ("bc5s normal", kind, name, off))
        _unchanged(u, src, ("bc5s normal", kind, name, off))


# ---- B. encode, host layer -----------------------------------------------------------------------------------------------------------------

def test_sliced_encode_steps_through_a_source_that_spans_4_gib(itw, gpu, oracle, arena):
    """itwCompressImageSlicedEx, slices of 4 rows of a 256 x 16 device source: every slice starts at ptr + stride * first row.  With a
    progress callback, and with one that stops the job at slice 2."""
    img = _ldr(16, 256, 11)
    want = _cpu_encode(oracle, "bc7", "veryfast", img, "sliced")
    v = _source(arena, img, COL)
    assert sp.crossings(16, sp.row_stride(v))[2] == [12, 13, 14, 15]       # the last slice starts beyond 2^32
    st = itw.bc7_profile("veryfast")
    calls = []
    ok, out = itw.compress_image("bc7", v, slice_pixels=4 * 256, settings=st, progress=lambda i, n, u: calls.append((i, n)) or True)
    _sync()
    assert ok and calls == [(1, 4), (2, 4), (3, 4)], calls
    _same_blocks(out, want, 16, "sliced")
    calls = []
    ok, out = itw.compress_image("bc7", v, slice_pixels=4 * 256, settings=st, progress=lambda i, n, u: calls.append(i) or i != 2)
    _sync()
    assert ok is False and calls == [1, 2] and itw.lib().itwLastError() is None
    _same_blocks(_host(out)[:2 * 64 * 16], want[:2 * 64 * 16], 16, "sliced, stopped at slice 2")
    _unchanged(v, img, "sliced")


def test_chain_encode_gathers_from_sources_that_span_4_gib(itw, gpu, oracle, arena):
    """itwCompressImageChainEx over three images: two sparse, one tight"""
    imgs = [_ldr(7, 1025, 12), _ldr(8, 260, 13), _ldr(16, 16, 14)]
    want = np.concatenate([oracle.encode_mt("bc1", itw.pad_to_multiple_of_4(np.array(a)), None) for a in imgs])
    views = [_source(arena, imgs[0], COL), _source(arena, imgs[1], 3 * COL), _dev(gpu, imgs[2])]
    ok, got = itw.compress_chain("bc1", views)
    _sync()
    assert ok
    _same_blocks(got, want, 8, "chain")
    for v, a in zip(views[:2], imgs):
        _unchanged(v, a, "chain")


def test_refine_rereads_a_source_that_spans_4_gib(itw, gpu, oracle, arena):
    import _refine as RF
    img = _ldr(8, 256, 15)
    _, first_errors = RF.tier(oracle, "bc7", "large offsets", img, "veryfast", 7)
    budget = int(np.median(first_errors))
    want = RF.predict(oracle, "bc7", "large offsets", img, "veryfast", "slow", 7, budget)
    assert 0 < want["listed"] < want["blocks"]
    v = _source(arena, img, COL)
    got = itw.compress_refined("bc7", v, "veryfast", "slow", budget, want_block_map=True, want_tier_map=True)
    _sync()
    RF.same(got, want, "refined")
    _unchanged(v, img, "refined")


def test_host_sources_that_span_4_gib_bc1_blocks(itw, gpu, oracle, host_arena):
    """CompressBlocksBC1 of a host surface: the pitched upload at a pitch of 0x30000000"""
    h, w = WHOLE
    img = _ldr(h, w, 1)
    v = _source(host_arena, img, COL)
    assert v.strides[0] == 0x30000000
    got = itw.compress_numpy("bc1", v)
    assert itw.lib().itwLastError() is None, itw.lib().itwLastError()
    _same_blocks(got, _cpu_encode(oracle, "bc1", None, img, WHOLE), 8, "host bc1")
    _unchanged(v, img, "host bc1")


def test_host_sources_that_span_4_gib_bc7_chain(itw, gpu, oracle, host_arena):
    """itwCompressImageChainEx of host images (copy_in)"""
    imgs = [_ldr(8, 260, 13), _ldr(7, 33, 16)]
    want = np.concatenate([oracle.encode_mt("bc7", itw.pad_to_multiple_of_4(np.array(a)), "basic") for a in imgs])
    views = [_source(host_arena, imgs[0], COL), _source(host_arena, imgs[1], 3 * COL)]
    ok, got = itw.compress_chain("bc7", views, profile="basic")
    assert ok, itw.last_error()
    _same_blocks(got, want, 16, "host chain")
    for v, a in zip(views, imgs):
        _unchanged(v, a, "host chain")


def _chain_views(buf, shapes, dtype, base=None, first_column=1):
    """one sparse view per level, each at its own column; level 0 holds `base`"""
    views = []
    for i, (h, w) in enumerate(shapes):
        col = (first_column + 2 * i) * COL
        views.append(_source(buf, base, col) if i == 0 and base is not None else _target(buf, h, w, dtype, col))
    return views


def _mip_shapes(h, w):
    out = [(h, w)]
    while h > 1 or w > 1:
        h, w = max(1, h >> 1), max(1, w >> 1)
        out.append((h, w))
    return out


def test_host_mip_levels_that_span_4_gib(itw, gpu, host_arena):
    """itwGenerateMipChain with host levels: the rows come back at the sparse stride (copy_out)"""
    import _mipgen as M
    base = _ldr(64, 64, 21)
    want = M.chain(base)
    views = _chain_views(host_arena, _mip_shapes(64, 64), np.uint8, base)
    itw.generate_mips_into([views])
    _unchanged(views[0], base, "host mips")
    for l, (v, wl) in enumerate(zip(views[1:], want[1:]), 1):
        _written(v, wl, ("host mips", l))


# ---- C. decode side ------------------------------------------------------------------------------------------------------------------------

DECODE = ["bc1", "bc3", "bc5", "bc7", "bc6h", "etc1", "bc2", "bc6h_signed"]
KEEPS_PARTIAL = ("bc5", "bc2")


def _stream(itw, gpu, oracle, fmt, sizes, seed):
    """(blocks, [texels], modes, min alpha per image) of a random stream.  bc1 .. bc6h: the oracle's from-spec decode
    (tests/test_gpu_decode_chain.py).  etc1, bc2 and the signed reading of bc6h: this library's decode into tight targets."""
    import test_gpu_decode_chain as DC
    if fmt in DC.FORMATS:
        blocks, want, modes = DC._case(itw, oracle, fmt, list(sizes), seed=seed)
        amin = [int(t[..., 3].view(np.uint8 if t.dtype == np.int8 else t.dtype).min()) for t in want]
        return np.array(blocks), want, modes, amin
    k = ("stream", fmt, tuple(sizes), seed)
    if k not in _refs:
        base = "bc6h" if fmt == "bc6h_signed" else fmt
        nb = sum(DC._nblocks(sizes))
        blocks = np.random.default_rng(900 + seed).integers(0, 256, nb * itw.BYTES_PER_BLOCK[base], dtype=np.uint8)
        outs, modes, amin = itw.decode_chain(fmt, _dev(gpu, blocks), list(sizes), want_modes=True, want_min_alpha=True)
        _sync()
        _refs[k] = (blocks, [_host(o).view(np.uint16 if base == "bc6h" else np.uint8) for o in outs], _host(modes),
                    [int(x) & 0xFFFFFFFF for x in amin.cpu().tolist()])
    return _refs[k]


def _texel_dtype(fmt):
    return np.uint16 if fmt.startswith("bc6h") else np.uint8


@pytest.mark.parametrize("fmt", DECODE)
def test_decode_image_into_a_target_that_spans_4_gib(itw, gpu, oracle, arena, fmt):
    """itwDecodeImage, 1025 x 7.  Expected: the oracle's decode; for etc1, bc2 and bc6h_signed the same call into a tight target."""
    blocks, want, want_modes, want_min = _stream(itw, gpu, oracle, fmt, [PARTIAL], 3)
    v = _target(arena, PARTIAL[0], PARTIAL[1], _texel_dtype(fmt), 7 * COL)
    _, modes, amin = itw.decode_image(fmt, _dev(gpu, blocks), v, want_modes=True, want_min_alpha=True)
    _sync()
    _written(v, want[0], ("decode image", fmt))
    assert np.array_equal(_host(modes), want_modes), fmt
    assert int(amin.cpu()[0]) & 0xFFFFFFFF == want_min[0], fmt


@pytest.mark.parametrize("fmt", DECODE)
def test_decode_blocks_into_a_target_that_spans_4_gib(itw, gpu, oracle, arena, fmt):
    """itwDecodeBlocks with out_stride = S: 1025 x 7 for the formats that keep partial blocks, 1028 x 8 for the others"""
    import torch
    size = PARTIAL if fmt in KEEPS_PARTIAL else WHOLE
    blocks, want, want_modes, _ = _stream(itw, gpu, oracle, fmt, [size], 4)
    v = _target(arena, size[0], size[1], _texel_dtype(fmt), 7 * COL)
    modes = torch.full((want_modes.size,), -9, dtype=torch.int32, device=gpu)
    itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
    rc = itw.lib().itwDecodeBlocks(itw.DXGI_FORMAT[fmt], C.c_void_p(_dev(gpu, blocks).data_ptr()), size[1], size[0], C.c_void_p(v.data_ptr()),
                                   sp.row_stride(v), C.c_void_p(modes.data_ptr()))
    _sync()
    assert rc == 0, itw.last_error()
    _written(v, want[0], ("decode blocks", fmt))
    assert np.array_equal(_host(modes), want_modes), fmt


@pytest.mark.parametrize("fmt", ["bc3", "bc6h"])
def test_decode_chain_into_two_targets_that_span_4_gib(itw, gpu, oracle, arena, fmt):
    sizes = [PARTIAL, (9, 37)]
    blocks, want, want_modes, want_min = _stream(itw, gpu, oracle, fmt, sizes, 5)
    views = [_target(arena, h, w, _texel_dtype(fmt), (7 + 4 * i) * COL) for i, (h, w) in enumerate(sizes)]
    _, modes, amin = itw.decode_chain(fmt, _dev(gpu, blocks), views, want_modes=True, want_min_alpha=True)
    _sync()
    for i, (v, w) in enumerate(zip(views, want)):
        _written(v, w, ("decode chain", fmt, i))
    assert np.array_equal(_host(modes), want_modes)
    assert [int(x) & 0xFFFFFFFF for x in amin.cpu().tolist()] == want_min


@pytest.mark.parametrize("fmt", ["bc1", "bc6h"])
def test_measure_against_a_source_that_spans_4_gib(itw, gpu, oracle, arena, fmt):
    """itwMeasureBlocks (stats and the per-block map) and itwMeasureChain, sources sparse"""
    import test_gpu_measure as TM
    sizes = [PARTIAL, (9, 37)]
    srcs = [TM._random_source(fmt, h, w, 40 + i) for i, (h, w) in enumerate(sizes)]
    nbs = [((w + 3) // 4) * ((h + 3) // 4) for h, w in sizes]
    bpb = itw.BYTES_PER_BLOCK[fmt]
    blocks = TM._random_blocks(itw, fmt, sum(nbs), 41)
    wants = [TM._expect(itw, oracle, fmt, blocks[:nbs[0] * bpb], srcs[0]), TM._expect(itw, oracle, fmt, blocks[nbs[0] * bpb:], srcs[1])]
    views = [_source(arena, s, (8 + 4 * i) * COL) for i, s in enumerate(srcs)]
    d_blocks = _dev(gpu, blocks)
    st, bmap = itw.measure(fmt, d_blocks, views[0], want_block_map=True)
    _sync()
    TM._same(st, wants[0][0], ("measure", fmt))
    assert np.array_equal(_host(bmap), wants[0][1]), ("block map", fmt)
    for i, s in enumerate(itw.measure_chain(fmt, d_blocks, views)):
        TM._same(s, wants[i][0], ("measure chain", fmt, i))
    for v, s in zip(views, srcs):
        _unchanged(v, s, ("measure", fmt))


@pytest.mark.parametrize("zoom,view_w,view_h,x,y", [(1.0, 70, 7, 960, 0), (3.0, 300, 2, 40, 0)])
def test_preview_of_a_surface_that_spans_4_gib(itw, gpu, arena, zoom, view_w, view_h, x, y):
    import _preview
    img = _ldr(7, 1025, 50)
    want = _preview.viewport(img, view_w, view_h, x, y, zoom, 4 + 8 + 16, 0x00C86432, 1.0)
    v = _source(arena, img, 2 * COL)
    got = itw.preview_surface(v, view_w, view_h, x=x, y=y, zoom=zoom, matte=0x00C86432)
    _sync()
    assert np.array_equal(_host(got), want), (zoom, int((_host(got) != want).any(axis=2).sum()))
    _unchanged(v, img, "preview")


# ---- D. texel stages -----------------------------------------------------------------------------------------------------------------------

def _run_mips(itw, arena, base, want, what, **options):
    shapes = [lv.shape[:2] for lv in want]
    views = _chain_views(arena, shapes, base.dtype, base)
    itw.generate_mips_into([views], **options)
    _sync()
    _unchanged(views[0], base, what)
    for l, (v, wl) in enumerate(zip(views[1:], want[1:]), 1):
        _written(v, wl, (what, "level", l))
    return views


@pytest.mark.parametrize("kind", ["rgba8", "rgba16f"])
@pytest.mark.parametrize("per_level", [False, True], ids=["pyramid", "per-level"])
def test_mip_chain_whose_levels_each_span_4_gib(itw, gpu, arena, kind, per_level):
    import _mipgen as M
    base = _ldr(64, 64, 60) if kind == "rgba8" else M.seeded_half_image(64, 64, 60)
    _run_mips(itw, arena, base, M.chain(base), ("mips", kind, per_level), per_level=per_level)


def test_srgb_mip_chain_whose_levels_each_span_4_gib(itw, gpu, arena):
    import _srgb_mips as SR
    base = _ldr(64, 64, 61)
    _run_mips(itw, arena, base, SR.chain(base), "srgb mips", srgb=True)


def test_linear_mip_chain_of_an_odd_size_whose_levels_each_span_4_gib(itw, gpu, arena):
    import _mipgen as M
    base = _ldr(21, 37, 62)
    _run_mips(itw, arena, base, M.chain(base), "linear mips 37 x 21")


@pytest.mark.parametrize("filt", ["cubic", "triangle"])
def test_cubic_and_triangle_mips_read_rows_across_a_4_gib_span(itw, gpu, arena, filt):
    """both wrap bits: the taps of the first and last rows reach the other end of the image"""
    import _mip_filters as MF
    base = MF.seeded_byte_image(21, 37, 63)
    _run_mips(itw, arena, base, MF.chain(base, filt, "uv", "rgba8"), ("mips", filt), filter=filt, wrap="uv")


@pytest.mark.parametrize("filt,addr", [("point", ""), ("linear", ""), ("cubic", "mirror"), ("triangle", "")])
def test_free_size_chain_whose_levels_each_span_4_gib(itw, gpu, arena, filt, addr):
    """ITW_MIP_RESIZE, 24 x 10 -> 40 x 17 -> 13 x 5"""
    import _mip_filters as MF
    import _resize as R
    sizes = ((24, 10), (40, 17), (13, 5))
    base = MF.seeded_byte_image(10, 24, 64)
    want = R.chain(base, sizes, filt, addr, "rgba8")
    views = _chain_views(arena, [(h, w) for w, h in sizes], np.uint8, base)
    itw.resize_chain_into([views], filter=filt, wrap="", mirror="uv" if addr == "mirror" else "")
    _sync()
    _unchanged(views[0], base, ("resize", filt))
    for l, (v, wl) in enumerate(zip(views[1:], want[1:]), 1):
        _written(v, wl, ("resize", filt, "level", l))


def test_alpha_mip_chain_and_coverage_whose_levels_each_span_4_gib(itw, gpu, arena):
    """itwGenerateMipChainAlpha with weight_colour and coverage_ref = 128, the report included; itwAlphaCoverage of a sparse image"""
    import _alpha_mips as A
    base = A.cutout(64, 64, 65)
    want, rows = A.chain(base, weight=True, ref=128)
    views = _chain_views(arena, [lv.shape[:2] for lv in want], np.uint8, base)
    _, report = itw.generate_mips_into([views], alpha_weight=True, alpha_coverage=128, report=True)
    _sync()
    assert [(int(r.texels), int(r.covered_plain), int(r.covered), int(r.threshold)) for r in report] == rows
    _unchanged(views[0], base, "alpha mips")
    for l, (v, wl) in enumerate(zip(views[1:], want[1:]), 1):
        _written(v, wl, ("alpha mips", l))
    assert itw.alpha_coverage(views[0], 128) == int(np.count_nonzero(base[..., 3] >= 128))
    assert itw.alpha_coverage(views[:4], 200) == [int(np.count_nonzero(lv[..., 3] >= 200)) for lv in want[:4]]


def test_normal_maps_prepared_in_place_across_a_4_gib_span(itw, gpu, arena):
    """itwPrepareNormalMapChain, both flips and the normalise"""
    import _normal_prep as N
    imgs = [_normal_img(7, 1025), _normal_img(8, 36)]
    views = [_source(arena, a, (1 + 4 * i) * COL) for i, a in enumerate(imgs)]
    itw.prepare_normal_map(views, ops=7)
    _sync()
    for v, a in zip(views, imgs):
        _written(v, np.ascontiguousarray(N.prepare(a, 7)), ("prepare", a.shape))


def test_normal_maps_quantized_between_surfaces_that_span_4_gib(itw, gpu, arena):
    """itwQuantizeNormalMapChain: float sources, int8 targets, both sparse"""
    import _normal_snorm as S
    imgs = [S.content("float", 7, 1025, 70), S.content("float", 8, 36, 71)]
    srcs = [_source(arena, a, (1 + 8 * i) * COL) for i, a in enumerate(imgs)]
    outs = [_target(arena, a.shape[0], a.shape[1], np.int8, (5 + 8 * i) * COL) for i, a in enumerate(imgs)]
    itw.quantize_normal_map(srcs, ops=7, out=outs)
    _sync()
    for s, o, a in zip(srcs, outs, imgs):
        _written(o, np.ascontiguousarray(S.quantize(a, 7)), ("quantize", a.shape))
        _unchanged(s, a, ("quantize", a.shape))


def _height_ops():
    import _height_normal as H
    return [("wrap", H.ops_word()), ("mirror", H.ops_word(5, True, True, True, True, 8.0, 7))]


@pytest.mark.parametrize("name,ops", _height_ops(), ids=["wrap", "mirror"])
def test_height_maps_to_normal_maps_across_a_4_gib_span(itw, gpu, arena, name, ops):
    """ITW_NORMAL_FROM_HEIGHT reads the rows above and below, under wrap the first and the last of the image: in place
    (itwPrepareNormalMapChain, RGBA8) and from float heights into int8 targets (itwQuantizeNormalMapChain), there with the source
    sparse and then with the target sparse"""
    import _height_normal as H
    a = H.content("uint8", 9, 37, 80)
    v = _source(arena, a, COL)
    itw.height_to_normal(v, ops, kind="biased")
    _sync()
    _written(v, H.to_rgba8(a, ops), ("height, biased", name))
    # source and target of this call may not interleave (the library compares their extents, first byte to last), so one of them is sparse
    # at a time and the other tight
    import torch
    f = H.content("float", 9, 37, 81)
    want = H.to_snorm(f, ops)
    s = _source(arena, f, 4 * COL)
    got = itw.height_to_normal(s, ops, kind="snorm", out=torch.zeros((9, 37, 4), dtype=torch.int8, device=gpu))
    _sync()
    assert np.array_equal(_host(got), want), ("height, snorm, sparse source", name)
    _unchanged(s, f, ("height, snorm", name))
    sp.reset(arena)
    o = _target(arena, 9, 37, np.int8, 8 * COL)
    itw.height_to_normal(_dev(gpu, f), ops, kind="snorm", out=o)
    _sync()
    _written(o, want, ("height, snorm, sparse target", name))


@pytest.mark.parametrize("pixel_size", [4, 8])
def test_pad_reads_a_source_that_spans_4_gib(itw, gpu, arena, pixel_size):
    """itwPadToMultipleOf4Device, 5 x 7"""
    import torch
    h, w = 7, 5
    img = _ldr(h, w, 90) if pixel_size == 4 else np.random.default_rng(91).integers(0, 65536, (h, w, 4), dtype=np.uint16)
    v = _source(arena, img, COL)
    out = torch.zeros((8, 8, 4), dtype=v.dtype, device=gpu)
    itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
    itw.lib().itwPadToMultipleOf4Device(C.byref(itw.RgbaSurface(v.data_ptr(), w, h, sp.row_stride(v))), pixel_size, C.c_void_p(out.data_ptr()))
    _sync()
    assert itw.lib().itwLastError() is None, itw.lib().itwLastError()
    assert np.array_equal(_host(out).view(img.dtype), np.pad(img, ((0, 1), (0, 3), (0, 0)), mode="edge"))
    _unchanged(v, img, ("pad", pixel_size))


# ---- last: nothing above may have been skipped on a device that had the memory ------------------------------------------------------------------

def test_no_large_offset_case_was_skipped(gpu, device_arena):
    import torch
    print(f"large-offset cases skipped: {len(_skipped)}; arena {ARENA_BYTES} bytes")
    if device_arena is None and torch.cuda.mem_get_info(gpu)[0] < 8 << 30:
        return                                                     # the device really is that full
    assert not _skipped, _skipped
