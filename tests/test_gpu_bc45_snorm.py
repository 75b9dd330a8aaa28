"""GPU, BC4_SNORM / BC5_SNORM (include/itw_bc45.h CompressBlocksBC4S / BC5S, DXGI 81 / 84): the encoders emit the bytes of the reference's
own D3DXEncodeBC4S / D3DXEncodeBC5S (tests/_dxtex_snorm.py: oracle/_ref/libdxtex_bc_ref.so, BC4BC5.cpp compiled unmodified), the decoders
and the measurement follow its D3DXDecodeBC4S / BC5S, and the layers around them treat the pair like BC4 / BC5.  Every comparison is
byte or integer equality."""
import ctypes as C
import os

import numpy as np
import pytest

import _dxtex_snorm as ref
from _guarded import frozen, guarded, rows_of
from conftest import first_mismatch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS = ["bc4_snorm", "bc5_snorm"]
NCH = {"bc4_snorm": 1, "bc5_snorm": 2}
BPB = {"bc4_snorm": 8, "bc5_snorm": 16}
_want = {}


def want_stream(fmt, key, img):
    """The reference's stream for `img`, computed once per (format, key) and shared."""
    k = (fmt, key)
    if k not in _want:
        _want[k] = ref.encode(NCH[fmt], img)
        _want[k].setflags(write=False)
    return _want[k]


def gpu_encode(itw, gpu, fmt, img):
    import torch
    out = itw.compress(fmt, torch.from_numpy(np.ascontiguousarray(img)).to(gpu))
    torch.cuda.synchronize()
    return out.cpu().numpy()


boundary_heavy_snorm = ref.boundary_heavy_snorm


def normal_map(h, w):
    from itw_amd import surfaces
    return surfaces.snorm_normal_map(h, w)


# ---- 1. the index function -----------------------------------------------------------------------------------------------------------

def test_device_index_function_is_the_first_strict_minimum_for_all_2_24_cases(itw, gpu):
    """itwTestBc45ClosestS runs the device function the encoders use -- run table plus the escape for the 30 pairs whose entry has more than
    8 runs -- for every (r0, r1, code).  F: the first index with the strictly smallest |level - t| over the reference decoder's levels."""
    F = ref.closest_table(ref.levels())
    got = np.full((256, 256, 256), 0xEE, dtype=np.uint8)
    assert itw.test_lib().itwTestBc45ClosestS(got.ctypes.data) == 0
    bad = np.argwhere(got != F)
    assert bad.size == 0, (len(bad), bad[:8], got[tuple(bad[0])], F[tuple(bad[0])])


# ---- 2. parity with D3DXEncodeBC4S / BC5S ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("h,w", [(512, 512), (53, 101), (1, 1), (3, 2), (4, 4), (9, 263)])
def test_normal_maps_vs_reference(itw, gpu, fmt, h, w):
    img = normal_map(h, w)
    got = gpu_encode(itw, gpu, fmt, img)
    want = want_stream(fmt, ("normal", h, w), img)
    assert got.size == want.size == itw.block_count(fmt, w, h) * BPB[fmt]
    assert first_mismatch(got, want, 8) is None, first_mismatch(got, want, 8)


@pytest.mark.parametrize("fmt", FMTS)
def test_boundary_value_content(itw, gpu, fmt):
    img = boundary_heavy_snorm()
    want = want_stream(fmt, "boundary", img)
    # on the reference's stream alone: both ramp forms well represented, and blocks on the pairs the run table cannot hold
    ends = want.reshape(-1, 8)[:, :2].view(np.int8).astype(np.int32)
    assert (ends[:, 0] <= ends[:, 1]).mean() > 0.2 and (ends[:, 0] > ends[:, 1]).mean() > 0.2
    escape = {7, 13, 14, 26, 27, 28, 29, 52, 53, 54, 55, 56, 57, 58, 59}
    assert sum(1 for a, b in ends if a == b and abs(a) in escape) >= 1
    got = gpu_encode(itw, gpu, fmt, img)
    assert first_mismatch(got, want, 8) is None, first_mismatch(got, want, 8)


def test_golden_streams(itw, gpu):
    """tests/golden/golden_bc45_snorm.npz (tools/gen_golden_bc45_snorm.py): seeded inputs and the reference's streams, needing no binary."""
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "golden_bc45_snorm.npz")))
    for name in ("normal_53x101", "boundary_128"):
        img = g[name + ".input"]
        assert img.dtype == np.int8
        for fmt in FMTS:
            got = gpu_encode(itw, gpu, fmt, img)
            assert first_mismatch(got, g[f"{name}.{fmt}"], 8) is None, (name, fmt, first_mismatch(got, g[f"{name}.{fmt}"], 8))


# ---- 3. flat and two-level blocks, every texel code -----------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FMTS)
def test_flat_and_two_level_blocks(itw, gpu, fmt):
    """Flat blocks of every code -128 .. 127 and blocks of two adjacent codes: equal endpoints are where the interpolated levels sit an
    ulp apart.  Codes -128 and -127 are the same value: their blocks must be the same bytes."""
    img = np.zeros((8, 256 * 4, 4), dtype=np.int8)
    for i, v in enumerate(range(-128, 128)):
        img[0:4, i * 4:i * 4 + 4, 0] = v
        img[0:4, i * 4:i * 4 + 4, 1] = v if i < 2 else -v             # (the first two: -128 and -127 in G as well)
        img[4:8, i * 4:i * 4 + 4, 0] = np.array([v, min(v + 1, 127)] * 8, dtype=np.int8).reshape(4, 4)
        img[4:8, i * 4:i * 4 + 4, 1] = np.array([v, max(v - 1, -128)] * 8, dtype=np.int8).reshape(4, 4)
    got = gpu_encode(itw, gpu, fmt, img)
    want = want_stream(fmt, "flat", img)
    assert first_mismatch(got, want, 8) is None, first_mismatch(got, want, 8)
    blocks = got.reshape(-1, BPB[fmt])
    assert np.array_equal(blocks[0], blocks[1])                    # the -128 block = the -127 block, every channel


@pytest.mark.parametrize("fmt", FMTS)
def test_every_texel_code_against_hand_picked_ramps(itw, gpu, fmt):
    """Two texels pin the ramp's ends, the other fourteen walk the range between them; the ends include -128, -127 and 127."""
    rng = np.random.default_rng(45)
    blocks = []
    for lo in list(range(-128, 128, 7)) + [-128, -127, -126, 126, 127]:
        for hi in (lo, min(lo + 1, 127), min(lo + 3, 127), min(lo + 17, 127), min(lo + 90, 127), 127):
            t = rng.integers(min(lo, hi), max(lo, hi) + 1, size=16)
            t[rng.integers(0, 16)] = lo
            t[rng.integers(0, 16)] = hi
            blocks.append(t)
    blocks = np.array(blocks, dtype=np.int8)
    n, cols = blocks.shape[0], 32
    rows = -(-n // cols)
    img = np.zeros((rows * 4, cols * 4, 4), dtype=np.int8)
    for i, t in enumerate(blocks):
        by, bx = divmod(i, cols)
        img[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4, 0] = t.reshape(4, 4)
        img[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4, 1] = t[::-1].reshape(4, 4)
    got = gpu_encode(itw, gpu, fmt, img)
    want = want_stream(fmt, "ramps", img)
    assert first_mismatch(got, want, 8) is None, first_mismatch(got, want, 8)


# ---- 4. host pointers and strides -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FMTS)
def test_host_pointers_and_strided_rows(itw, gpu, fmt):
    import torch
    img = np.ascontiguousarray(normal_map(64, 72)[:61, :70])
    want = want_stream(fmt, "61x70", img)
    assert first_mismatch(itw.compress_numpy(fmt, img), want, 8) is None
    wide = np.zeros((61, 75, 4), np.int8)                         # pitch 300 B: rows not 16-byte aligned -> the dword loads
    wide[:, 3:73] = img
    assert first_mismatch(itw.compress_numpy(fmt, wide[:, 3:73]), want, 8) is None
    t = torch.from_numpy(wide).to(gpu)[:, 3:73]                   # device-resident, strided, base offset 12 B
    out = itw.compress(fmt, t)
    torch.cuda.synchronize()
    assert first_mismatch(out.cpu().numpy(), want, 8) is None
    assert torch.equal(out, itw.compress(fmt, t.contiguous()))


# ---- 5. the persistent walk -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,th,tw,ry,rx", [("bc5_snorm", 208, 256, 10, 8), ("bc4_snorm", 1028, 256, 4, 8)])
def test_persistent_walk_takes_a_second_chunk(itw, gpu, fmt, th, tw, ry, rx):
    """A workgroup takes a second chunk only above 2048 x 256 = 524 288 channel blocks: 2048 x 2080 BC5S has 532 480, 2048 x 4112 BC4S
    526 336.  Blocks are independent, so the tiled surface encodes to the tile's stream repeated; the tile equals the reference."""
    import torch
    bpb = BPB[fmt]
    tile = normal_map(th, tw)
    want = want_stream(fmt, ("tile", th, tw), tile)
    base = torch.from_numpy(tile).to(gpu)
    small = itw.compress(fmt, base)
    torch.cuda.synchronize()
    assert first_mismatch(small.cpu().numpy(), want, 8) is None
    big = base.repeat(ry, rx, 1).contiguous()
    assert (big.shape[0] // 4) * (big.shape[1] // 4) * NCH[fmt] > 2048 * 256
    out = itw.compress(fmt, big).view(ry * th // 4, rx * tw // 4, bpb)
    torch.cuda.synchronize()
    s2 = small.view(th // 4, tw // 4, bpb)
    for i in range(ry):
        for j in range(rx):
            assert torch.equal(out[th // 4 * i:th // 4 * (i + 1), tw // 4 * j:tw // 4 * (j + 1)], s2), (i, j)
    sub = big[8:8 + 4 * 333, 16:16 + 4 * 401]
    assert torch.equal(itw.compress(fmt, sub), itw.compress(fmt, sub.contiguous()))


# ---- 6. decode ------------------------------------------------------------------------------------------------------------------------

def _random_blocks(nch, n, seed):
    """Every endpoint value, -128 included, on both sides; random indices."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, size=(n * nch, 8), dtype=np.uint8)
    if n * nch >= 768:
        ends = np.arange(-128, 128).astype(np.int8).view(np.uint8)
        b[:256, 0] = ends
        b[256:512, 1] = ends
        b[512:768, 0] = ends
        b[512:768, 1] = ends                                      # equal endpoints
    else:
        b[0, 0], b[1, 1], b[2, :2] = 0x80, 0x80, 0x80             # -128 on either side and on both
    return b.reshape(n, 8 * nch)


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_is_the_integer_rule_and_the_rounded_reference(itw, gpu, fmt):
    import torch
    nch = NCH[fmt]
    cases = [(want_stream(fmt, ("normal", 53, 101), normal_map(53, 101)), 101, 53),
             (want_stream(fmt, "boundary", boundary_heavy_snorm()), 128, 128),
             (_random_blocks(nch, 4096, 81 + nch).reshape(-1), 256, 256),
             (_random_blocks(nch, 6, 7).reshape(-1), 10, 6)]       # 3 x 2 blocks, cropped to 10 x 6
    for blocks, w, h in cases:
        got = itw.decode(fmt, torch.from_numpy(np.array(blocks)).to(gpu), w, h)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert got.dtype == np.int8 and got.shape == (h, w, 4)
        rule = ref.decode_int8(nch, blocks, w, h)
        assert np.array_equal(got, rule), np.argwhere(got != rule)[:4]
        fl = ref.decode(nch, blocks)                                               # (n, 16, 4) floats of D3DXDecodeBC4S / BC5S
        by, bx = (h + 3) // 4, (w + 3) // 4
        full = np.rint(127.0 * fl.astype(np.float64)).astype(np.int32).reshape(by, bx, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(by * 4, bx * 4, 4)
        assert np.array_equal(got[..., :nch].astype(np.int32), full[:h, :w, :nch])
        assert (got[..., nch:3] == 0).all() and (got[..., 3] == 127).all() and got.min() >= -127
        assert np.array_equal(itw.decode(fmt, np.array(blocks), w, h), got)        # host pointers


# ---- 7. measure -----------------------------------------------------------------------------------------------------------------------

def _expect_stats(nch, blocks, src):
    h, w = src.shape[:2]
    dec = ref.decode_int8(nch, blocks, w, h).astype(np.int64)
    s = np.maximum(src.astype(np.int64), -127)                                     # -128 and -127 both mean -1.0
    d = s - dec
    by, bx = (h + 3) // 4, (w + 3) // 4
    sq = np.zeros((by * 4, bx * 4), dtype=np.int64)
    sq[:h, :w] = (d * d).sum(axis=2)
    bsse = sq.reshape(by, 4, bx, 4).sum(axis=(1, 3)).reshape(-1)
    return {"sse": [int(v) for v in (d * d).sum(axis=(0, 1))], "max_abs": [int(v) for v in np.abs(d).max(axis=(0, 1))],
            "worst_block_sse": int(bsse.max()), "worst_block": int(np.argmax(bsse)), "blocks": by * bx}, bsse


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("h,w", [(64, 64), (6, 10)])
def test_measure_equals_numpy_on_the_decoded_int8_surface(itw, gpu, fmt, h, w):
    import torch
    nch = NCH[fmt]
    rng = np.random.default_rng(h * 100 + w + nch)
    src = normal_map(64, 64)[:h, :w].copy()
    blocks = ref.encode(nch, src) if (h, w) != (64, 64) else np.array(want_stream(fmt, ("normal64",), src))
    src[rng.integers(0, h, 24), rng.integers(0, w, 24), rng.integers(0, 4, 24)] = -128      # after encoding: the measurement's own rule
    src[0, 0, 2] = 100                                                                       # a filled channel that differs
    want, bsse = _expect_stats(nch, blocks, src)
    for dev in (True, False):
        b = torch.from_numpy(blocks).to(gpu) if dev else blocks
        s = torch.from_numpy(src).to(gpu) if dev else src
        st, bmap = itw.measure(fmt, b, s, want_block_map=True)
        bmap = bmap.cpu().numpy() if dev else bmap
        got = st.as_dict()
        assert (got["dxgi_format"], got["width"], got["height"]) == (itw.DXGI_FORMAT[fmt], w, h)
        for k, v in want.items():
            assert got[k] == v, (k, got[k], v)
        assert got["mode_hist"] == [want["blocks"]] + [0] * 15 and got["reserved_blocks"] == 0
        assert np.array_equal(np.asarray(bmap).astype(np.int64), bsse)
        assert max(got["max_abs"]) <= 254
        mask = 3 if nch == 2 else 1
        total = sum(want["sse"][c] for c in range(nch))
        psnr = itw.lib().itwStatsPsnr(C.byref(st), mask)
        assert total > 0 and abs(psnr - 10.0 * np.log10(254.0 * 254.0 * (w * h * nch) / total)) <= 1e-9


# ---- 8. layers ------------------------------------------------------------------------------------------------------------------------

def _mips(img):
    """A chain down to 1 x 1 by dropping every other row and column (the content of the levels is not what is tested)."""
    out = [np.ascontiguousarray(img)]
    while out[-1].shape[0] > 1 or out[-1].shape[1] > 1:
        a = out[-1]
        lv = np.empty((max(1, a.shape[0] // 2), max(1, a.shape[1] // 2), 4), dtype=a.dtype)     # (fresh: plain row-major strides at 1 x 1 too)
        lv[...] = a[::2, ::2][:lv.shape[0], :lv.shape[1]]
        out.append(lv)
    return out


@pytest.mark.parametrize("fmt", FMTS)
def test_chain_and_measure_chain(itw, gpu, fmt):
    import torch
    nch = NCH[fmt]
    levels = _mips(normal_map(64, 64))
    assert [lv.shape[0] for lv in levels] == [64, 32, 16, 8, 4, 2, 1]
    want = np.concatenate([ref.encode(nch, lv) for lv in levels])
    assert itw.chain_bytes(fmt, levels) == want.size
    ok, got = itw.compress_chain(fmt, levels)
    assert ok and first_mismatch(got, want, 8) is None, first_mismatch(got, want, 8)
    ok, dgot = itw.compress_chain(fmt, [torch.from_numpy(lv).to(gpu) for lv in levels])
    torch.cuda.synchronize()
    assert ok and np.array_equal(dgot.cpu().numpy(), want)
    ok, fgot = itw.compress_chain(fmt, levels, cmp_func=itw.image_func(fmt))
    assert ok and np.array_equal(fgot, want)
    stats = itw.measure_chain(fmt, want, levels)
    off = 0
    for lv, st in zip(levels, stats):
        n = itw.block_count(fmt, lv.shape[1], lv.shape[0]) * BPB[fmt]
        exp, _ = _expect_stats(nch, want[off:off + n], lv)
        got_d = st.as_dict()
        for k, v in exp.items():
            assert got_d[k] == v, (lv.shape, k, got_d[k], v)
        off += n


@pytest.mark.parametrize("multithreaded", [False, True])
def test_compress_image_through_the_trampoline(itw, gpu, multithreaded):
    """CompressImageBC5S through the slice loop (4 slices of a 64 x 72 image) and CompressImageST / MT."""
    img = np.ascontiguousarray(normal_map(72, 64))
    want = want_stream("bc5_snorm", "72x64", img)
    calls = []
    ok, got = itw.compress_image("bc5_snorm", img, multithreaded=multithreaded, slice_pixels=64 * 72 // 4,
                                 progress=lambda i, n, _: calls.append((i, n)) or True)
    assert ok and first_mismatch(got, want, 8) is None, first_mismatch(got, want, 8)
    assert calls and calls[-1][1] == 4
    ok, got4 = itw.compress_image("bc4_snorm", img[:70, :61].copy(), multithreaded=multithreaded)
    assert ok and first_mismatch(got4, ref.encode(1, img[:70, :61].copy()), 8) is None
    with pytest.raises(ValueError):
        itw.compress_refined("bc5_snorm", img, "fast", "slow", 100)


# ---- 9. write extents -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("h,w", [(7, 9), (64, 64)])
def test_outputs_lie_between_their_guards(itw, gpu, fmt, h, w):
    import torch
    nch = NCH[fmt]
    img = np.ascontiguousarray(normal_map(64, 64)[:h, :w])
    want = ref.encode(nch, img)
    src = frozen(img, row_pad=12, device=gpu)
    out = guarded(want.size, device=gpu)
    with torch.cuda.device(gpu):
        itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
        surf = itw.RgbaSurface(src.ptr, w, h, src.stride)
        getattr(itw.lib(), "CompressBlocksBC4S" if nch == 1 else "CompressBlocksBC5S")(C.byref(surf), out.ptr)
    torch.cuda.synchronize()
    assert np.array_equal(out.host(), want)
    out.check("encode")
    src.check("encode source")
    # decode into a strided surface
    stride = w * 4 + 20
    dec = guarded(h * stride, device=gpu, rows=(h, w * 4, stride))
    blk = frozen(want, device=gpu)
    assert itw.lib().itwDecodeBlocks(itw.DXGI_FORMAT[fmt], blk.ptr, w, h, dec.ptr, stride, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(rows_of(dec, np.int8).reshape(h, w, 4), ref.decode_int8(nch, want, w, h))
    dec.check("decode")
    blk.check("decode blocks")
    # measure: stats and the block map
    nb = itw.block_count(fmt, w, h)
    stats = guarded(C.sizeof(itw.ErrorStats), device=gpu, offset=8)
    bmap = guarded(nb * 8, device=gpu)
    assert itw.lib().itwMeasureBlocks(itw.DXGI_FORMAT[fmt], blk.ptr, C.byref(surf), stats.ptr, C.sizeof(itw.ErrorStats), bmap.ptr) == 0
    torch.cuda.synchronize()
    exp, bsse = _expect_stats(nch, want, img)
    st = itw.ErrorStats.from_buffer_copy(stats.host().tobytes())
    assert [int(v) for v in st.sse] == exp["sse"] and int(st.blocks) == nb
    assert np.array_equal(bmap.host().view(np.uint64).astype(np.int64), bsse)
    stats.check("measure stats")
    bmap.check("measure map")
    src.check("measure source")
    blk.check("measure blocks")


# ---- 10. graph capture ----------------------------------------------------------------------------------------------------------------

def test_device_call_is_capturable_after_warmup(itw, gpu):
    """After itwWarmupBC45S() a device-pointer call is one kernel launch on the stream: captured once, replayed to the same bytes."""
    import torch
    itw.lib().itwWarmupBC45S()
    assert itw.last_error() is None
    d = torch.from_numpy(normal_map(64, 64)).to(gpu)
    want = itw.compress("bc5_snorm", d)
    torch.cuda.synchronize()
    want = want.clone()
    assert np.array_equal(want.cpu().numpy(), want_stream("bc5_snorm", ("normal64",), normal_map(64, 64)))
    out = torch.zeros_like(want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        itw.compress("bc5_snorm", d, out=out)
    torch.cuda.synchronize()
    for replays in (1, 3):
        out.zero_()
        for _ in range(replays):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), replays
    assert itw.last_error() is None
