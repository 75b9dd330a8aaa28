"""itwCompressImageRefined (include/itw_dispatch.h): a cheap preset everywhere, an expensive one only on the blocks whose error is above a
budget.  Every expected byte -- target, error map, tier map, the seven stats fields -- comes from the CPU oracle alone (tests/_refine.py:
both presets over the whole image, the errors of both from the oracle's decoders in numpy int64, then the rule); every comparison is ==."""
import ctypes as C

import numpy as np
import pytest

import _refine as R

pytestmark = pytest.mark.gpu

_content = {}


def _img(golden_inputs, key):
    """Test content by name, built once and frozen."""
    if key not in _content:
        if key == "photo":                                       # a 64 x 64 crop of the reference's baboon.png (opaque)
            img = np.ascontiguousarray(golden_inputs["baboon"][96:160, 64:128])
        elif key == "photo_alpha":                               # ... with random alpha, for the mask
            img = np.ascontiguousarray(golden_inputs["baboon"][96:160, 64:128])
            img[..., 3] = np.random.default_rng(15).integers(0, 256, size=(64, 64), dtype=np.uint8)
        elif key == "noise_alpha":
            img = np.random.default_rng(7).integers(0, 256, size=(64, 64, 4), dtype=np.uint8)
        elif key == "hdr":                                       # a crop of the HDR golden input, alpha plane set to random bits
            img = np.ascontiguousarray(golden_inputs["monkey_hdr"][80:144, 80:144])
            img[..., 3] = np.random.default_rng(6).integers(0, 65536, size=(64, 64), dtype=np.uint16)
        elif key == "noise_576":                                 # 128 x 72: 32 x 18 = 576 blocks, three workgroups, the last partial
            img = np.random.default_rng(1).integers(0, 256, size=(72, 128, 4), dtype=np.uint8)
        elif key == "bench_1024":
            from itw_amd import surfaces
            img = surfaces.ldr_smooth(1024, 1024, seed=surfaces.SEED)
        img.setflags(write=False)
        _content[key] = img
    return _content[key]


def _median_budget(oracle, fmt, key, img, first, mask):
    return int(np.median(R.tier(oracle, fmt, key, img, first, mask)[1]))


def _run(itw, gpu, fmt, img, first, refine, budget, channels):
    import torch
    got = itw.compress_refined(fmt, R.to_gpu(gpu, img), first, refine, budget, channels=channels, want_block_map=True, want_tier_map=True)
    torch.cuda.synchronize()
    return got


PARITY = [("bc7", "photo", "veryfast", "slow", 7), ("bc7", "photo", "ultrafast", "basic", 7), ("bc7", "noise_alpha", "alpha_veryfast", "alpha_slow", 15),
          ("bc6h", "hdr", "veryfast", "slow", 7), ("bc6h", "hdr", "fast", "veryslow", 7)]
CHANNELS = {7: "rgb", 15: "rgba"}


@pytest.mark.parametrize("fmt,key,first,refine,mask", PARITY, ids=[f"{f}-{a}-{b}" for f, k, a, b, m in PARITY])
def test_parity_with_the_oracle_rule(itw, gpu, oracle, golden_inputs, fmt, key, first, refine, mask):
    """64 x 64: 256 blocks, one workgroup; the budget is the median of the oracle's first-tier map."""
    img = _img(golden_inputs, key)
    budget = _median_budget(oracle, fmt, key, img, first, mask)
    want = R.predict(oracle, fmt, key, img, first, refine, mask, budget)
    assert 0 < want["listed"] < 256
    R.same(_run(itw, gpu, fmt, img, first, refine, budget, CHANNELS[mask]), want, (fmt, first, refine))


def test_parity_cases_include_a_refinement_that_loses(oracle, golden_inputs):
    """CPU side: at least one parity case lists blocks of which some, not all, take the second encoding."""
    partial = []
    for fmt, key, first, refine, mask in PARITY:
        img = _img(golden_inputs, key)
        want = R.predict(oracle, fmt, key, img, first, refine, mask, _median_budget(oracle, fmt, key, img, first, mask))
        partial.append(0 < want["replaced"] < want["listed"])
    assert any(partial), partial


LISTED = [0, 1, 63, 64, 65, 255, 256, 257, 576]


@pytest.mark.parametrize("count", LISTED)
def test_list_edges(itw, gpu, oracle, golden_inputs, count):
    """BC7 ultrafast -> veryfast on 128 x 72 noise: 32 x 18 = 576 blocks, three workgroups of the judge, the last one partial.  Budgets
    from the oracle's sorted map list exactly `count` blocks: none, one, a wave and a workgroup boundary from either side, 257 = a second
    row of the packed surface, all."""
    img = _img(golden_inputs, "noise_576")
    ea = R.tier(oracle, "bc7", "noise_576", img, "ultrafast", 7)[1]
    s = np.sort(ea)
    assert s[0] > 0                                              # budget 0 lists every block
    budget = 0 if count == 576 else int(s[576 - count - 1])
    assert count in (0, 576) or s[576 - count - 1] < s[576 - count]   # no tie at this rank
    want = R.predict(oracle, "bc7", "noise_576", img, "ultrafast", "veryfast", 7, budget)
    assert want["listed"] == count
    got = _run(itw, gpu, "bc7", img, "ultrafast", "veryfast", budget, "rgb")
    R.same(got, want, count)
    assert np.array_equal(got[3].cpu().numpy() == 0, ea <= budget)   # tier 0 exactly off the list


def test_equal_tiers_keep_the_first(itw, gpu, oracle, golden_inputs):
    img = _img(golden_inputs, "photo")
    budget = _median_budget(oracle, "bc7", "photo", img, "veryfast", 7)
    a, ea = R.tier(oracle, "bc7", "photo", img, "veryfast", 7)
    got = _run(itw, gpu, "bc7", img, "veryfast", "veryfast", budget, "rgb")
    R.same(got, R.predict(oracle, "bc7", "photo", img, "veryfast", "veryfast", 7, budget), "ties")
    assert got[1].replaced == 0 and got[1].listed > 0
    assert np.array_equal(got[0].cpu().numpy().reshape(-1, 16), a)
    assert np.array_equal(got[3].cpu().numpy(), (ea > budget).astype(np.uint8))      # 1 on the list


def test_a_losing_refinement_never_raises_a_block_error(itw, gpu, oracle, golden_inputs):
    img = _img(golden_inputs, "photo")
    ea = R.tier(oracle, "bc7", "photo", img, "slow", 7)[1]
    budget = int(np.median(ea))
    got = _run(itw, gpu, "bc7", img, "slow", "ultrafast", budget, "rgb")
    R.same(got, R.predict(oracle, "bc7", "photo", img, "slow", "ultrafast", 7, budget), "slow -> ultrafast")
    assert (got[2].cpu().numpy() <= ea).all()


def test_nothing_listed(itw, gpu, oracle, golden_inputs):
    img = _img(golden_inputs, "photo")
    a, ea = R.tier(oracle, "bc7", "photo", img, "veryfast", 7)
    got = _run(itw, gpu, "bc7", img, "veryfast", "slow", R.U64_MAX, "rgb")
    R.same(got, R.predict(oracle, "bc7", "photo", img, "veryfast", "slow", 7, R.U64_MAX), "UINT64_MAX")
    assert np.array_equal(got[0].cpu().numpy().reshape(-1, 16), a)
    assert got[1].listed == 0 and got[1].sse_final == got[1].sse_first == int(ea.sum())


def test_channel_mask(itw, gpu, oracle, golden_inputs):
    """An RGB preset on a source with random alpha: the alpha differences count with mask 15 only."""
    import torch
    img = _img(golden_inputs, "photo_alpha")
    budget = _median_budget(oracle, "bc7", "photo_alpha", img, "veryfast", 7)
    got = {}
    for mask in (7, 15):
        want = R.predict(oracle, "bc7", "photo_alpha", img, "veryfast", "slow", mask, budget)
        got[mask] = _run(itw, gpu, "bc7", img, "veryfast", "slow", budget, CHANNELS[mask])
        R.same(got[mask], want, ("mask", mask))
    t7, t15 = got[7][3].cpu().numpy(), got[15][3].cpu().numpy()
    assert 0 < (t7 > 0).sum() < 256 and not np.array_equal(t7 > 0, t15 > 0)
    st, bmap = itw.measure("bc7", got[15][0], R.to_gpu(gpu, img), want_block_map=True)
    torch.cuda.synchronize()
    assert torch.equal(bmap, got[15][2]) and sum(int(v) for v in st.sse) == got[15][1].sse_final


def _raw(itw, fmt, src, w, h, stride, first, refine, mask, budget, target, stats, bmap, tmap):
    """The C call on addresses (ints): for pointer kinds the binding does not mix."""
    s1, s2 = itw.bc7_profile(first), itw.bc7_profile(refine)
    surf = itw.RgbaSurface(src, w, h, stride)
    ok = itw.lib().itwCompressImageRefined(C.byref(surf), target, itw.DXGI_FORMAT[fmt], C.addressof(s1), C.addressof(s2), mask, budget,
                                           stats, C.sizeof(itw.RefineStats), bmap, tmap)
    assert ok, itw.last_error()


def test_pointer_kinds(itw, gpu, oracle, golden_inputs):
    """All host pointers, all device pointers (stats too), and a device source whose rows are 48 bytes apart from tight: the same bytes."""
    import torch
    from _guarded import frozen
    img = _img(golden_inputs, "noise_576")
    h, w = img.shape[:2]
    budget = int(np.median(R.tier(oracle, "bc7", "noise_576", img, "ultrafast", 7)[1]))
    want = R.predict(oracle, "bc7", "noise_576", img, "ultrafast", "veryfast", 7, budget)
    R.same(itw.compress_refined("bc7", img, "ultrafast", "veryfast", budget, want_block_map=True, want_tier_map=True), want, "all host")
    itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
    tight, strided = R.to_gpu(gpu, img), frozen(img, row_pad=48, device=gpu)
    for what, ptr, stride in (("all device", tight.data_ptr(), w * 4), ("strided device source", strided.ptr, strided.stride)):
        out = torch.zeros(576 * 16, dtype=torch.uint8, device=gpu)
        stats = torch.zeros(C.sizeof(itw.RefineStats), dtype=torch.uint8, device=gpu)
        bmap = torch.zeros(576, dtype=torch.int64, device=gpu)
        tmap = torch.full((576,), 9, dtype=torch.uint8, device=gpu)
        torch.cuda.synchronize()
        _raw(itw, "bc7", ptr, w, h, stride, "ultrafast", "veryfast", 7, budget, out.data_ptr(), stats.data_ptr(), bmap.data_ptr(), tmap.data_ptr())
        st = itw.RefineStats.from_buffer_copy(stats.cpu().numpy().tobytes())
        R.same((out, st, bmap, tmap), want, what)
    strided.check("strided device source")


def test_several_packed_rows(itw, gpu, oracle, golden_inputs):
    """1024 x 1024 of the bench content, BC7 veryfast -> slow, the budget at the oracle's 70th percentile: about 19 000 listed blocks,
    77 rows of the packed surface, 256 workgroups of the judge (the oracle takes about 7 s on 8 cores for the two encodings)."""
    img = _img(golden_inputs, "bench_1024")
    ea = R.tier(oracle, "bc7", "bench_1024", img, "veryfast", 7, mt=True)[1]
    budget = int(np.sort(ea)[int(ea.size * 0.7)])
    want = R.predict(oracle, "bc7", "bench_1024", img, "veryfast", "slow", 7, budget, mt=True)
    assert 15000 < want["listed"] < 23000 and 0 < want["replaced"]
    R.same(_run(itw, gpu, "bc7", img, "veryfast", "slow", budget, "rgb"), want, "1024^2")


def test_example_refine_option(oracle, gpu, tmp_path):
    """examples/encode_dds --refine <profile> <max_block_sse>: one line with the call's statistics on stdout, the refined stream in the file."""
    import os
    import subprocess
    from itw_amd import surfaces
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "encode_dds")
    img = surfaces.ldr_smooth(64, 64)
    want = R.predict(oracle, "bc7", "ldr_smooth_64", img, "veryfast", "slow", 7, 300)
    assert 0 < want["replaced"] and want["listed"] > 0
    raw, dds = tmp_path / "in.raw", tmp_path / "out.dds"
    img.tofile(raw)
    r = subprocess.run([exe, "--refine", "slow", "300", "bc7_veryfast", "64", "64", str(raw), str(dds)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip() == ("refined: bc7_veryfast -> slow budget 300 blocks {blocks} listed {listed} replaced {replaced} sse {sse_first} -> {sse_final} "
                                "worst {worst_first} -> {worst_final}").format(**want)
    assert np.array_equal(np.fromfile(dds, dtype=np.uint8)[-256 * 16:].reshape(-1, 16), want["target"])
