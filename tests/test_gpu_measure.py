"""itwMeasureBlocks / itwMeasureChain (include/itw_decode.h): the fused decode + compare + reduce kernel against the from-spec CPU
decoders of the oracle.  Expected values: oracle.decode at the padded size, cropped to the source, BC6H's alpha fill applied (as in
test_gpu_decode.py), compared in numpy int64.  Every quantity is an integer, so every comparison is `==`, except PSNR (1e-9 dB)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("dxgi_format", "width", "height", "reserved_blocks", "blocks", "sse", "max_abs", "worst_block_sse", "worst_block", "mode_hist")


def _oracle_texels(oracle, fmt, blocks, w, h):
    dec, modes = oracle.decode(fmt, blocks, w, h)
    if fmt == "bc6h":
        full = np.empty((h, w, 4), dtype=np.uint16)
        full[..., :3] = dec
        full[..., 3] = 0x3C00
        dec = full
    return dec, modes


def _expect(itw, oracle, fmt, blocks, src):
    """The reference: (dict of the fields of itw_error_stats, per-block sums) of the stream `blocks` against the texels `src`."""
    h, w = src.shape[:2]
    H, W = (h + 3) // 4 * 4, (w + 3) // 4 * 4
    nb = (H // 4) * (W // 4)
    blocks = np.ascontiguousarray(blocks).reshape(-1)[: nb * itw.BYTES_PER_BLOCK[fmt]]
    dec, modes = _oracle_texels(oracle, fmt, blocks, W, H)
    d = src.astype(np.int64) - dec[:h, :w].astype(np.int64)
    sq = d * d
    per_texel = np.zeros((H, W), dtype=np.int64)
    per_texel[:h, :w] = sq.sum(axis=2)
    bmap = per_texel.reshape(H // 4, 4, W // 4, 4).sum(axis=(1, 3)).reshape(-1)
    assert (modes >= -1).all()
    want = {"dxgi_format": itw.DXGI_FORMAT[fmt], "width": w, "height": h, "reserved_blocks": int((modes == -1).sum()), "blocks": nb,
            "sse": [int(v) for v in sq.sum(axis=(0, 1))], "max_abs": [int(v) for v in np.abs(d).max(axis=(0, 1))],
            "worst_block_sse": int(bmap.max()), "worst_block": int(np.argmax(bmap)),            # argmax: the first index of the maximum
            "mode_hist": [int(v) for v in np.bincount(modes[modes >= 0], minlength=16)]}
    return want, bmap


def _same(stats, want, what=""):
    got = stats.as_dict()
    for f in FIELDS:
        assert got[f] == want[f], (what, f, got[f], want[f])
    assert stats._pad == 0


def _random_blocks(itw, fmt, nblocks, seed):
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 256, size=nblocks * itw.BYTES_PER_BLOCK[fmt], dtype=np.uint8)
    if fmt == "bc7":                                             # spread the unary mode prefix evenly, incl. reserved
        b = blocks.reshape(-1, 16)
        for i in range(b.shape[0]):
            m = i % 9
            b[i, 0] = (int(b[i, 0]) & (0xff & ~((1 << min(m + 1, 8)) - 1))) | ((1 << m) & 0xff)
    return blocks


def _random_source(fmt, h, w, seed):
    rng = np.random.default_rng(1000 + seed)
    if fmt == "bc6h":
        return rng.integers(0, 65536, size=(h, w, 4), dtype=np.uint16)
    return rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)


def _to_gpu(gpu, a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(gpu)


def _measure_on_device(itw, gpu, fmt, blocks, src):
    import torch
    st, bmap = itw.measure(fmt, _to_gpu(gpu, blocks), _to_gpu(gpu, src), want_block_map=True)
    torch.cuda.synchronize()
    return st, bmap.cpu().numpy()


@pytest.mark.parametrize("fmt", ["bc1", "bc3", "bc4", "bc5", "bc7", "bc6h"])
def test_random_bits_every_format(itw, gpu, oracle, fmt):
    w, h = 128, 64                                               # 512 blocks: two workgroups
    seed = {"bc1": 1, "bc3": 3, "bc4": 4, "bc5": 5, "bc7": 7, "bc6h": 6}[fmt]
    blocks = _random_blocks(itw, fmt, 512, seed)
    src = _random_source(fmt, h, w, seed)
    want, want_map = _expect(itw, oracle, fmt, blocks, src)
    st, bmap = _measure_on_device(itw, gpu, fmt, blocks, src)
    _same(st, want, fmt)
    assert np.array_equal(bmap, want_map)
    assert sum(want["mode_hist"]) + want["reserved_blocks"] == 512
    if fmt == "bc7":
        assert all(v > 0 for v in want["mode_hist"][:8]) and want["reserved_blocks"] > 0
    if fmt == "bc6h":
        assert sum(1 for v in want["mode_hist"][:14] if v) >= 10 and want["reserved_blocks"] > 0
    if fmt in ("bc1", "bc3", "bc4", "bc5"):
        assert want["mode_hist"][0] == 512


@pytest.mark.parametrize("w", [4, 260, 1028])                    # 1 block; 65: one lane into a second wave; 257: one lane into a second workgroup
def test_reduction_edges(itw, gpu, oracle, w):
    blocks = _random_blocks(itw, "bc7", w // 4, w)
    src = _random_source("bc7", 4, w, w)
    want, want_map = _expect(itw, oracle, "bc7", blocks, src)
    st, bmap = _measure_on_device(itw, gpu, "bc7", blocks, src)
    _same(st, want, w)
    assert np.array_equal(bmap, want_map)


@pytest.mark.parametrize("fmt,w,h", [("bc7", 5, 3), ("bc7", 1, 1), ("bc1", 5, 3), ("bc1", 1, 1), ("bc4", 61, 62), ("bc5", 9, 5)])
def test_partial_sizes_compare_only_the_crop(itw, gpu, oracle, fmt, w, h):
    from itw_amd import surfaces
    img = np.ascontiguousarray(surfaces.ldr_smooth(64, 64)[:h, :w])
    ok, stream = itw.compress_chain(fmt, [img], profile="basic" if fmt == "bc7" else None)      # a one-image chain: ceil(w/4)*ceil(h/4) blocks
    assert ok and stream.size == ((w + 3) // 4) * ((h + 3) // 4) * itw.BYTES_PER_BLOCK[fmt]
    want, want_map = _expect(itw, oracle, fmt, stream, img)
    st, bmap = itw.measure(fmt, stream, img, want_block_map=True)                                 # host pointers
    _same(st, want, "encoder's stream, host")
    assert np.array_equal(bmap.astype(np.int64), want_map)
    dst, dmap = _measure_on_device(itw, gpu, fmt, stream, img)
    _same(dst, want, "encoder's stream, device")
    assert np.array_equal(dmap, want_map)
    # The encoder fills the padding of an edge block with copies of the image's own texels, so a kernel that wrongly compared padding
    # texels could still pass above.  Random blocks decode to padding texels that match nothing: only the w x h crop may count.
    noise = _random_blocks(itw, fmt, stream.size // itw.BYTES_PER_BLOCK[fmt], 31 * w + h)
    want, want_map = _expect(itw, oracle, fmt, noise, img)
    st, bmap = _measure_on_device(itw, gpu, fmt, noise, img)
    _same(st, want, "random blocks")
    assert np.array_equal(bmap, want_map)
    assert sum(want["sse"]) > 0


def test_strided_source_measures_like_the_contiguous_copy(itw, gpu, oracle):
    import torch
    blocks = _random_blocks(itw, "bc3", 256, 11)
    wide = _random_source("bc3", 64, 96, 11)
    view = wide[:, 16:80]                                        # 64 x 64 texels, rows 96 texels apart, starting 64 B into a row
    want, _ = _expect(itw, oracle, "bc3", blocks, np.ascontiguousarray(view))
    d_wide = _to_gpu(gpu, wide)
    d_blocks = _to_gpu(gpu, blocks)
    strided = itw.measure("bc3", d_blocks, d_wide[:, 16:80])
    contiguous = itw.measure("bc3", d_blocks, d_wide[:, 16:80].contiguous())
    torch.cuda.synchronize()
    _same(strided, want, "strided")
    assert strided == contiguous
    odd = itw.measure("bc3", d_blocks, d_wide[:, 17:81])         # rows that are not 16-byte aligned take the dword loads
    want_odd, _ = _expect(itw, oracle, "bc3", blocks, np.ascontiguousarray(wide[:, 17:81]))
    _same(odd, want_odd, "unaligned rows")
    host = itw.measure("bc3", blocks, view)                      # a strided host surface is staged row by row
    _same(host, want, "strided host")


def test_sums_beyond_32_bits_bc1(itw, gpu, oracle):
    """2048^2 white blocks against an all-zero source: 2048^2 * 255^2 per channel, above 2^32."""
    import torch
    size = 2048
    nb = (size // 4) ** 2
    white = np.array([0xff, 0xff, 0xff, 0xff, 0, 0, 0, 0], dtype=np.uint8)      # c0 == c1 == 0xFFFF, every index 0: opaque white
    one, _ = oracle.decode("bc1", white, 4, 4)
    assert (one == 255).all()
    d_blocks = torch.from_numpy(np.tile(white, nb)).to(gpu)
    d_src = torch.zeros((size, size, 4), dtype=torch.uint8, device=gpu)
    st, bmap = itw.measure("bc1", d_blocks, d_src, want_block_map=True)
    torch.cuda.synchronize()
    per_channel = size * size * 255 * 255
    assert per_channel > 2 ** 32
    _same(st, {"dxgi_format": 71, "width": size, "height": size, "reserved_blocks": 0, "blocks": nb, "sse": [per_channel] * 4,
               "max_abs": [255] * 4, "worst_block_sse": 64 * 255 * 255, "worst_block": 0, "mode_hist": [nb] + [0] * 15})
    assert int((bmap != 64 * 255 * 255).sum().item()) == 0


def test_sums_beyond_32_bits_bc6h_one_block(itw, gpu, oracle):
    """One BC6H block against a zero source, chosen so that one lane's per-channel sum exceeds 2^32."""
    blocks = _random_blocks(itw, "bc6h", 64, 66).reshape(-1, 16)
    zero = np.zeros((4, 4, 4), dtype=np.uint16)
    picked = None
    for i in range(blocks.shape[0]):
        want, want_map = _expect(itw, oracle, "bc6h", blocks[i], zero)
        if max(want["sse"]) > 2 ** 32:
            picked = i
            break
    assert picked is not None
    st, bmap = _measure_on_device(itw, gpu, "bc6h", blocks[picked].copy(), zero)
    _same(st, want, picked)
    assert np.array_equal(bmap, want_map)
    assert want["sse"][3] == 16 * 0x3C00 ** 2                    # the alpha fill is measured like any channel


def test_ties_go_to_the_first_block(itw, gpu, oracle):
    """A constant source, a stream that reproduces it exactly except for three identical bad blocks: the first one is reported."""
    w = h = 128                                                  # 1024 blocks: four workgroups
    white = np.array([0xff, 0xff, 0xff, 0xff, 0, 0, 0, 0], dtype=np.uint8)
    black = np.zeros(8, dtype=np.uint8)                          # c0 == c1 == 0, index 0: opaque black
    blocks = np.tile(white, 1024).reshape(-1, 8)
    for b in (3, 200, 700):
        blocks[b] = black
    src = np.full((h, w, 4), 255, dtype=np.uint8)
    want, want_map = _expect(itw, oracle, "bc1", blocks.reshape(-1), src)
    assert want["worst_block"] == 3 and want["worst_block_sse"] == 48 * 255 * 255 and sorted(np.nonzero(want_map)[0]) == [3, 200, 700]
    st, bmap = _measure_on_device(itw, gpu, "bc1", blocks.reshape(-1), src)
    _same(st, want)
    assert st.worst_block == 3
    assert np.array_equal(bmap, want_map)
    blocks[3] = white                                            # ... and without block 3, the next one in raster order
    st = itw.measure("bc1", _to_gpu(gpu, blocks.reshape(-1)), _to_gpu(gpu, src))
    assert st.worst_block == 200 and st.worst_block_sse == 48 * 255 * 255


@pytest.mark.parametrize("key,fmt,channels", [("baboon.bc1", "bc1", "rgb"), ("baboon.bc7.slow", "bc7", "rgba"), ("monkey_hdr.bc6h.slow", "bc6h", None)])
def test_real_encoder_output(itw, gpu, oracle, golden_blocks, golden_inputs, key, fmt, channels):
    import torch
    blocks = np.ascontiguousarray(golden_blocks[key]).reshape(-1)
    src = golden_inputs[key.split(".")[0]]
    src = np.ascontiguousarray(src.view(np.uint16) if fmt == "bc6h" else src)
    want, want_map = _expect(itw, oracle, fmt, blocks, src)
    host, host_map = itw.measure(fmt, blocks, src, want_block_map=True)
    _same(host, want, "host pointers")
    assert np.array_equal(host_map.astype(np.int64), want_map)
    dev, dev_map = _measure_on_device(itw, gpu, fmt, blocks, src)
    assert dev == host and np.array_equal(dev_map, want_map)
    assert want["reserved_blocks"] == 0
    if fmt == "bc6h":
        with pytest.raises(ValueError):
            host.psnr()
        return
    picked = ["rgba".index(c) for c in channels]
    total = np.float64(sum(want["sse"][c] for c in picked))
    psnr = 10.0 * np.log10(np.float64(255.0 ** 2) * np.float64(src.shape[0] * src.shape[1] * len(picked)) / total)
    assert abs(host.psnr(channels) - float(psnr)) <= 1e-9 and host.psnr() == host.psnr(channels)
    assert 20.0 < psnr < 60.0                                    # an encoding of the image, not of something else


def test_chain_measures_each_level_like_the_single_call(itw, gpu, oracle):
    import torch
    from itw_amd import surfaces
    levels = itw.mip_chain(surfaces.ldr_smooth(1023, 517))
    assert len(levels) == 10
    ok, stream = itw.compress_chain("bc7", levels, profile="veryfast")
    assert ok
    host = itw.measure_chain("bc7", stream, levels)
    dev = itw.measure_chain("bc7", _to_gpu(gpu, stream), [_to_gpu(gpu, lv) for lv in levels])
    torch.cuda.synchronize()
    assert len(host) == len(dev) == 10
    off = 0
    for i, lv in enumerate(levels):
        n = ((lv.shape[1] + 3) // 4) * ((lv.shape[0] + 3) // 4) * 16
        alone = itw.measure("bc7", stream[off:off + n], lv)
        assert host[i] == alone and dev[i] == alone, i
        assert (alone.width, alone.height) == (lv.shape[1], lv.shape[0])
        if i >= 3:                                               # the small levels against the oracle as well (partial sizes down to 1 x 1)
            _same(alone, _expect(itw, oracle, "bc7", stream[off:off + n], lv)[0], i)
        off += n
    assert off == stream.size


def test_a_captured_measurement_replays_over_changed_inputs(itw, gpu, oracle):
    """All four pointers on the device: the call is plain asynchronous work on the caller's stream (zero, measure, finish: one branch),
    allocates nothing and can be captured; each replay measures what the buffers hold then."""
    import torch
    w, h = 128, 64
    inputs = [(_random_blocks(itw, "bc7", 512, 90 + i), _random_source("bc7", h, w, 90 + i)) for i in range(3)]
    d_blocks = _to_gpu(gpu, inputs[0][0])
    d_src = _to_gpu(gpu, inputs[0][1])
    d_stats = torch.zeros(C.sizeof(itw.ErrorStats), dtype=torch.uint8, device=gpu)
    d_map = torch.zeros(512, dtype=torch.int64, device=gpu)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        itw.measure_async("bc7", d_blocks, d_src, d_stats, d_map)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        itw.measure_async("bc7", d_blocks, d_src, d_stats, d_map)
    torch.cuda.synchronize()
    for blocks, src in inputs[1:]:
        d_blocks.copy_(torch.from_numpy(blocks))
        d_src.copy_(torch.from_numpy(src))
        d_stats.fill_(0xEE)                                      # every field is written by the replay
        d_map.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want, want_map = _expect(itw, oracle, "bc7", blocks, src)
        _same(itw.stats_from_tensor(d_stats), want)
        assert np.array_equal(d_map.cpu().numpy(), want_map)
    assert itw.last_error() is None


@pytest.mark.parametrize("name,fmt,h,w", [("bc7_basic", "bc7", 61, 70), ("bc5", "bc5", 37, 30), ("bc6h_fast", "bc6h", 30, 41)])
def test_the_example_host_reports_what_its_file_costs(itw, gpu, oracle, tmp_path, name, fmt, h, w):
    """examples/encode_dds --measure: one line per image on stdout, the numbers of the blocks it wrote against the texels it read."""
    import os
    import re
    import subprocess
    from itw_amd import surfaces
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "encode_dds")
    img = np.ascontiguousarray((surfaces.hdr_smooth(64, 72) if fmt == "bc6h" else surfaces.ldr_smooth(64, 72))[:h, :w])
    raw, dds = tmp_path / "in.raw", tmp_path / "out.dds"
    img.tofile(raw)
    r = subprocess.run([exe, "--measure", name, str(w), str(h), str(raw), str(dds)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    f = np.fromfile(dds, dtype=np.uint8)
    d = itw.DdsDesc()
    off = itw.lib().itwDdsReadHeader(f.ctypes.data, f.size, C.byref(d))
    want, _ = _expect(itw, oracle, fmt, f[off:], img)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith(f"image 0: {w}x{h} {name}")
    m = re.search(r"sse \[(\d+), (\d+), (\d+), (\d+)\] max_abs \[(\d+), (\d+), (\d+), (\d+)\]", lines[0])
    assert [int(v) for v in m.groups()] == want["sse"] + want["max_abs"]
    p = re.search(r"psnr ([0-9.]+|inf) dB", lines[0])
    if fmt == "bc6h":
        assert p is None
    else:
        own = {"bc7": (0, 1, 2), "bc5": (0, 1)}[fmt]           # bc7_basic is an RGB preset
        psnr = 10 * np.log10(255.0 ** 2 * w * h * len(own) / sum(want["sse"][c] for c in own))
        assert abs(float(p.group(1)) - psnr) < 1e-4              # four decimals are printed
