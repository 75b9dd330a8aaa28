"""itwCompressImageChain[Ex] (include/itw_dispatch.h): a whole mip chain / cube map in one call.

"Expected" is what the plugin's per-image loop (IntelPlugin.cpp:229-255) produces, image after image: the pad to multiples of 4 then the
CPU oracle for BC1/BC3/BC6H/BC7, the oracle's DirectXTex encoder on the unpadded image for BC4/BC5.  For chains larger than a group
budget the per-image loop of this library's own calls (compress_image: oracle-pinned elsewhere) is the reference instead."""
import ctypes as C

import numpy as np
import pytest

from conftest import first_mismatch

pytestmark = pytest.mark.gpu

BPB = {"bc1": 8, "bc3": 16, "bc4": 8, "bc5": 16, "bc6h": 16, "bc7": 16}


def _content(fmt, h, w, seed=0):
    from itw_amd import surfaces
    return surfaces.hdr_smooth(h, w, seed=seed + 11) if fmt == "bc6h" else surfaces.ldr_smooth(h, w, seed=seed + 11)


def _oracle_chain(itw, oracle, fmt, levels, prof):
    parts = []
    for lv in levels:
        if fmt in ("bc4", "bc5"):
            parts.append(oracle.encode_bc45(fmt, lv))
        else:
            parts.append(oracle.encode_mt(fmt, itw.pad_to_multiple_of_4(lv), prof))
    return np.concatenate(parts)


def _per_image(itw, fmt, levels, prof):
    """The per-image loop of this library's own calls: pad (ISPC formats) then one compress_image per image."""
    parts = []
    for lv in levels:
        src = lv if fmt in ("bc4", "bc5") else itw.pad_to_multiple_of_4(lv)
        ok, out = itw.compress_image(fmt, src, prof)
        assert ok
        parts.append(out)
    return np.concatenate(parts)


def _host(out):
    return out.cpu().numpy() if hasattr(out, "cpu") else np.asarray(out)


def _check(got, want, fmt, what):
    got = _host(got)
    assert got.size == want.size, (what, got.size, want.size)
    m = first_mismatch(got, want, BPB[fmt])
    assert m is None, (what, m)


CHAINS = [("bc1", None, (1000, 600)), ("bc1", None, (1023, 517)), ("bc3", None, (1023, 517)), ("bc4", None, (1023, 517)),
          ("bc5", None, (1000, 600)), ("bc4", None, (37, 1)), ("bc5", None, (1023, 517)),
          ("bc7", "veryfast", (1000, 600)), ("bc7", "basic", (1023, 517)), ("bc7", "slow", (1023, 517)),
          ("bc7", "alpha_basic", (1000, 600)), ("bc7", "alpha_slow", (517, 301)),
          ("bc6h", "fast", (1000, 600)), ("bc6h", "slow", (1023, 517))]


@pytest.mark.parametrize("fmt,prof,size", CHAINS, ids=[f"{f}-{p or '-'}-{s[0]}x{s[1]}" for f, p, s in CHAINS])
def test_full_2d_chain_equals_the_per_image_oracle(itw, gpu, oracle, fmt, prof, size):
    import torch
    levels = itw.mip_chain(_content(fmt, *size))
    want = _oracle_chain(itw, oracle, fmt, levels, prof)
    assert itw.chain_bytes(fmt, levels) == want.size
    ok, got = itw.compress_chain(fmt, levels, prof)                                   # host pointers: what the plugin passes
    assert ok
    _check(got, want, fmt, "host")
    dev = [torch.from_numpy(lv).to(gpu) for lv in levels]                              # device-resident, device target
    ok, got = itw.compress_chain(fmt, dev, prof)
    torch.cuda.synchronize()
    assert ok
    _check(got, want, fmt, "device")


@pytest.mark.parametrize("fmt,prof,key", [("bc7", "basic", "bc7"), ("bc6h", "slow", "bc6h")])
def test_cube_map_chain_is_the_dds_of_the_per_image_calls(itw, gpu, oracle, fmt, prof, key):
    size = 256 if fmt == "bc7" else 128
    faces = [itw.mip_chain(_content(fmt, size, size, seed=f)) for f in range(6)]
    images = [lv for face in faces for lv in face]                                    # DDS order: face, then mip
    per_image = [_per_image(itw, fmt, [lv], prof) for lv in images]
    want = itw.dds_file(key, size, size, per_image, mip_levels=len(faces[0]), cubemap=True)
    ok, got = itw.compress_chain(fmt, images, prof)
    assert ok
    ends = np.cumsum([p.size for p in per_image])
    pieces = np.split(_host(got), ends[:-1])
    mine = itw.dds_file(key, size, size, pieces, mip_levels=len(faces[0]), cubemap=True)
    assert mine.size == want.size and first_mismatch(mine[-ends[-1]:], want[-ends[-1]:], BPB[fmt]) is None
    assert np.array_equal(mine, want)
    # and the first face against the oracle directly
    _check(_host(got)[:sum(p.size for p in per_image[:len(faces[0])])], _oracle_chain(itw, oracle, fmt, faces[0], prof), fmt, "face 0 vs oracle")


@pytest.mark.parametrize("fmt,prof,size", [("bc7", "basic", (2048, 2048)), ("bc1", None, (4096, 4096)), ("bc7", "basic", (2048, 2050)),
                                            ("bc6h", "slow", (1030, 1024)), ("bc4", None, (2051, 1024))])
def test_chains_larger_than_a_group(itw, gpu, fmt, prof, size):
    """Several groups, the in-place path of big aligned levels, and big unaligned levels gathered as a group of their own."""
    import torch
    levels = itw.mip_chain(_content(fmt, *size))
    want = _per_image(itw, fmt, levels, prof)
    ok, got = itw.compress_chain(fmt, levels, prof)
    assert ok
    _check(got, want, fmt, "host")
    dev = [torch.from_numpy(lv).to(gpu) for lv in levels]
    ok, got = itw.compress_chain(fmt, dev, prof, out=np.zeros(want.size, np.uint8))  # device images, host target
    assert ok
    _check(got, want, fmt, "device -> host")


def _strided_views(levels, pad):
    views = []
    for lv in levels:
        h, w = lv.shape[:2]
        base = np.full((h, w + pad, 4), 7, dtype=lv.dtype)
        base[:, :w] = lv
        views.append(base[:, :w])
    return views


def _scratch_image(levels):
    """All images in one contiguous allocation, one after another, like a DirectXTex ScratchImage (offsets need not be 16-B aligned)."""
    total = sum(lv.nbytes for lv in levels)
    buf = np.empty(total, dtype=np.uint8)
    views, off = [], 0
    for lv in levels:
        v = buf[off:off + lv.nbytes].view(lv.dtype).reshape(lv.shape)
        v[...] = lv
        views.append(v)
        off += lv.nbytes
    return buf, views


@pytest.mark.parametrize("fmt,prof", [("bc7", "basic"), ("bc6h", "fast"), ("bc4", None), ("bc1", None)])
def test_pointer_kinds_and_layouts(itw, gpu, oracle, fmt, prof):
    import torch
    levels = itw.mip_chain(_content(fmt, 301, 517))
    want = _oracle_chain(itw, oracle, fmt, levels, prof)
    ok, got = itw.compress_chain(fmt, _strided_views(levels, 13), prof)              # host rows longer than the image
    assert ok
    _check(got, want, fmt, "host, strided rows")
    buf, views = _scratch_image(levels)
    ok, got = itw.compress_chain(fmt, views, prof)                                   # one contiguous host allocation
    assert ok
    _check(got, want, fmt, "host, one allocation")
    dbuf = torch.from_numpy(buf).to(gpu)                                               # ... and on the device: unaligned image starts
    off, dev = 0, []
    for lv in levels:
        n = lv.nbytes
        t = dbuf[off:off + n]
        dev.append(t.view(torch.int16 if fmt == "bc6h" else torch.uint8).view(lv.shape))
        off += n
    ok, got = itw.compress_chain(fmt, dev, prof)
    torch.cuda.synchronize()
    assert ok
    _check(got, want, fmt, "device, one allocation")
    ok, got = itw.compress_chain(fmt, [torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for v in levels], prof, out=np.zeros(want.size, np.uint8))
    assert ok
    _check(got, want, fmt, "device images, host target")
    dstr = []
    for lv in levels:                                                                  # device rows with a stride that is no multiple of 16 B
        h, w = lv.shape[:2]
        base = torch.zeros((h, w + 3, 4), dtype=torch.int16 if fmt == "bc6h" else torch.uint8, device=gpu)
        base[:, :w] = torch.from_numpy(lv.view(np.int16) if fmt == "bc6h" else lv).to(gpu)
        dstr.append(base[:, :w])
    ok, got = itw.compress_chain(fmt, dstr, prof)
    torch.cuda.synchronize()
    assert ok
    _check(got, want, fmt, "device, strided rows")


@pytest.mark.parametrize("fmt,prof", [("bc7", "slow"), ("bc1", None), ("bc5", None), ("bc6h", "slow")])
def test_one_image_equals_the_ordinary_call_and_the_trampoline_equals_ex(itw, gpu, fmt, prof):
    img = _content(fmt, 260, 300)
    ok, want = itw.compress_image(fmt, img, prof)
    assert ok
    ok, got = itw.compress_chain(fmt, [img], prof)
    assert ok
    _check(got, want, fmt, "count = 1")
    levels = itw.mip_chain(_content(fmt, 130, 77))
    ok, ex = itw.compress_chain(fmt, levels, prof)
    assert ok
    ok, tr = itw.compress_chain(fmt, levels, cmp_func=itw.image_func(fmt, prof))
    assert ok
    _check(tr, _host(ex), fmt, "trampoline vs Ex")


def test_a_callers_own_function_gets_the_literal_loop(itw, gpu, oracle):
    levels = itw.mip_chain(_content("bc3", 67, 45))
    seen = []

    def mine(surf, out):
        s = surf.contents
        seen.append((s.width, s.height))
        itw.lib().CompressBlocksBC3(surf, out)

    fn = itw.abi.COMPRESSION_FUNC(mine)
    ok, got = itw.compress_chain("bc3", levels, cmp_func=C.cast(fn, C.c_void_p))
    assert ok
    assert seen == [((lv.shape[1] + 3) & ~3, (lv.shape[0] + 3) & ~3) for lv in levels]          # padded, once per image, in order
    _check(got, _oracle_chain(itw, oracle, "bc3", levels, None), "bc3", "literal loop")


@pytest.mark.parametrize("where", ["host", "device"])
def test_progress_is_called_for_every_image_in_order_and_stops_the_job(itw, gpu, oracle, where):
    import torch
    faces = [itw.mip_chain(_content("bc7", 256, 256, seed=f)) for f in range(6)]
    levels = [lv for face in faces for lv in face]
    n = len(levels)
    want = _oracle_chain(itw, oracle, "bc7", levels, "veryfast")
    ends = np.cumsum([((lv.shape[0] + 3) // 4) * ((lv.shape[1] + 3) // 4) * 16 for lv in levels])
    src = levels if where == "host" else [torch.from_numpy(lv).to(gpu) for lv in levels]
    calls = []
    ok, got = itw.compress_chain("bc7", src, "veryfast", progress=lambda i, t, u: calls.append((i, t)) or True)
    assert ok and calls == [(i, n) for i in range(1, n + 1)]
    _check(got, want, "bc7", "with progress")
    for k in (1, 2, n // 2, n):
        calls = []

        def prog(i, t, u):
            calls.append(i)
            return i != k

        ok, got = itw.compress_chain("bc7", src, "veryfast", progress=prog)
        assert ok is False and calls == list(range(1, k + 1)), (k, calls)
        written = int(ends[k - 2]) if k >= 2 else 0
        assert first_mismatch(_host(got)[:written], want[:written], 16) is None, k


def test_mixed_host_and_device_images_are_rejected(itw, gpu):
    import torch
    a = _content("bc1", 64, 64)
    b = torch.from_numpy(_content("bc1", 32, 32)).to(gpu)
    itw.set_error_mode(itw.ON_ERROR_RETURN)
    try:
        itw.lib().itwClearError()
        ok, _ = itw.compress_chain("bc1", [a, b], out=np.zeros(4096, np.uint8))
        assert ok is False and "host" in (itw.last_error() or "")
        itw.lib().itwClearError()
        ok, _ = itw.compress_chain("bc1", [a, b], out=np.zeros(4096, np.uint8), cmp_func=itw.image_func("bc1"))
        assert ok is False and itw.last_error()
    finally:
        itw.set_error_mode(itw.ON_ERROR_ABORT)
        itw.lib().itwClearError()


def _variants(fmt, size, n):
    """n distinct images of one size, cheaply: one surface rolled along both axes (a group that read another group's texels would show)."""
    base = _content(fmt, size, size)
    return [np.ascontiguousarray(np.roll(base, (37 * k, 91 * k), axis=(0, 1))) for k in range(n)]


@pytest.mark.parametrize("fmt,prof,size", [("bc1", None, 1450), ("bc7", "basic", 1026)])
def test_more_groups_than_the_event_ring(itw, gpu, fmt, prof, size):
    """Ten images, each a gather group of its own: more than half a window's budget each (BC1: 363^2 = 131 769 blocks, two make 263 538 >
    262 144; BC7 `basic`: 257^2 = 66 049, two make 132 098 > 131 072), below the budget, and no multiple of 4, so none is encoded in place.
    Ten groups wrap the ring of 8 input / done events and alternate the two kernel streams and workspace slices five times."""
    import torch
    images = _variants(fmt, size, 10)
    want = _per_image(itw, fmt, images, prof)
    ok, got = itw.compress_chain(fmt, images, prof)
    assert ok
    _check(got, want, fmt, "host")
    dev = [torch.from_numpy(im).to(gpu) for im in images]
    ok, got = itw.compress_chain(fmt, dev, prof, out=np.zeros(want.size, np.uint8))  # device images, host target
    assert ok
    _check(got, want, fmt, "device -> host")


def test_one_workspace_across_formats_and_streams(itw, gpu, oracle):
    """The per-thread workspace is shared by BC7 and BC6H and ordered across streams by a library-owned event: a device-resident BC7 call on
    stream A, a BC6H `slow` call on stream B, BC7 on A again, one synchronisation at the end, every stream against the oracle.
    Surface: 4 x 4 texels, one block -- the smallest for which both bc7_workspace_bytes (non-zero from the first block on: 4 B + 32 B per
    block in the deep shape) and bc6h_workspace_bytes (non-zero for `slow` settings -- slow_mode with fastSkipTreshold >= 2 -- from one
    block up to the wide shape's limit) are non-zero; below it there is no block and both are zero."""
    import torch
    from itw_amd import surfaces
    ldr = np.ascontiguousarray(surfaces.ldr_smooth(8, 8)[2:6, 1:5])
    ldr2 = np.ascontiguousarray(surfaces.ldr_smooth(8, 8, seed=5)[:4, 4:8])
    hdr = np.ascontiguousarray(surfaces.hdr_smooth(8, 8)[1:5, 3:7])
    d_ldr, d_ldr2, d_hdr = (torch.from_numpy(a).to(gpu) for a in (ldr, ldr2, hdr))
    a, b = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(a):
        first = itw.compress("bc7", d_ldr, "slow")
    with torch.cuda.stream(b):
        second = itw.compress("bc6h", d_hdr, "slow")
    with torch.cuda.stream(a):
        third = itw.compress("bc7", d_ldr2, "basic")
    torch.cuda.synchronize()
    itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
    _check(first, oracle.encode("bc7", ldr, "slow").reshape(-1), "bc7", "bc7 on stream A")
    _check(second, oracle.encode("bc6h", hdr, "slow").reshape(-1), "bc6h", "bc6h on stream B")
    _check(third, oracle.encode("bc7", ldr2, "basic").reshape(-1), "bc7", "bc7 on stream A again")
