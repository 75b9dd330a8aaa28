"""itwCompressImageRefinedTo (include/itw_dispatch.h): the device picks the budget -- from a number of blocks (policy A: one exact
(k+1)-th-largest select over the first tier's error map) or from a summed error to reach (policy B: up to five rounds).  Every expected
byte and every stats field comes from the CPU oracle alone (tests/_refine_target.py: np.sort for the select, a plain simulation of the
rounds); every comparison is ==.  Content as in tests/test_gpu_refine.py, whose frozen images (and so the oracle's cached encodings)
are shared."""
import ctypes as C

import numpy as np
import pytest

import _refine as R
import _refine_target as T
from test_gpu_refine import _img

pytestmark = pytest.mark.gpu

U = T.U64_MAX
_content = {}


def _own(golden_inputs, key):
    """Content this file adds, built once and frozen."""
    if key not in _content:
        if key == "noise_153":                                   # 68 x 36: 17 x 9 = 153 blocks, one partial workgroup
            img = np.random.default_rng(2).integers(0, 256, size=(36, 68, 4), dtype=np.uint8)
        elif key == "noise_2304":                                # 192 x 192: 2304 blocks, a second workgroup of the select's histogram pass
            img = np.random.default_rng(3).integers(0, 256, size=(192, 192, 4), dtype=np.uint8)
        elif key == "tiled":                                     # one 16 x 16 patch of the photo, 4 x 4 times: every error occurs 16 times
            img = np.tile(_img(golden_inputs, "photo")[16:32, 24:40], (4, 4, 1))
        elif key == "solid":
            img = np.empty((64, 64, 4), dtype=np.uint8)
            img[...] = (96, 160, 32, 255)
        elif key == "half_noise":
            # BC6H: every channel, alpha too, a random half code in [0, 0x7BFF].  Per block one random code `top`; each channel of each
            # texel is 0 or `top`: more corners of the colour cube than two regions fit, and an error that follows the block's swing
            rng = np.random.default_rng(4)
            top = rng.integers(0, 0x7C00, size=(16, 1, 16, 1, 1))
            img = (rng.integers(0, 2, size=(16, 4, 16, 4, 4)) * top).astype(np.uint16).reshape(64, 64, 4)
        img = np.ascontiguousarray(img)
        img.setflags(write=False)
        _content[key] = img
    return _content[key]


def _run(itw, gpu, fmt, img, first, refine, channels="rgb", **policy):
    import torch
    got = itw.compress_refined_to(fmt, R.to_gpu(gpu, img), first, refine, channels=channels, want_block_map=True, want_tier_map=True, **policy)
    torch.cuda.synchronize()
    return got


CHANNELS = {7: "rgb", 15: "rgba"}


def _policy_a(itw, gpu, oracle, fmt, key, img, first, refine, k, mask=7):
    """One policy A call against the prediction AND against itwCompressImageRefined called with the budget it chose; returns the prediction."""
    import torch
    want = T.predict(oracle, fmt, key, img, first, refine, mask, max_listed=k)
    got = _run(itw, gpu, fmt, img, first, refine, channels=CHANNELS[mask], max_listed=k)
    T.same(got, want, (key, k))
    ref = itw.compress_refined(fmt, R.to_gpu(gpu, img), first, refine, int(got[1].budget[0]), channels=CHANNELS[mask], want_block_map=True,
                               want_tier_map=True)
    torch.cuda.synchronize()
    assert torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3]), (key, k)
    assert bytes(got[1].total) == bytes(ref[1]), (key, k)
    return want


EDGES = [0, 1, 63, 64, 65, 255, 256, 257, 575, 576, 577, U]


@pytest.mark.parametrize("k", EDGES)
def test_select_edges(itw, gpu, oracle, golden_inputs, k):
    """BC7 ultrafast -> veryfast on 128 x 72 noise: 576 blocks, three workgroups of the count and list kernels, the last one partial.
    Ranks at none, one, a wave and a workgroup boundary from either side, the last block from either side, past the end."""
    img = _img(golden_inputs, "noise_576")
    ea = R.tier(oracle, "bc7", "noise_576", img, "ultrafast", 7)[1]
    s = np.sort(ea)[::-1]
    assert s[-1] > 0                                             # T = 0 lists every block
    want = _policy_a(itw, gpu, oracle, "bc7", "noise_576", img, "ultrafast", "veryfast", k)
    assert want["budget"][0] == (int(s[k]) if k < 576 else 0)
    assert want["listed"] == int((ea > want["budget"][0]).sum()) <= min(k, 576)
    if k >= 576 or s[k] < s[k - 1] or k == 0:                    # no tie at this rank: exactly min(k, 576) blocks
        assert want["listed"] == min(k, 576)


@pytest.mark.parametrize("k", [0, 1, 64, 152, 153, 154])
def test_a_single_partial_workgroup(itw, gpu, oracle, golden_inputs, k):
    img = _own(golden_inputs, "noise_153")
    _policy_a(itw, gpu, oracle, "bc7", "noise_153", img, "ultrafast", "veryfast", k)


@pytest.mark.parametrize("k", [1, 1000, 2047, 2048, 2049, 2303, 2304])
def test_a_second_histogram_workgroup(itw, gpu, oracle, golden_inputs, k):
    """192 x 192 noise: 2304 blocks, so the select's histogram pass (2048 blocks per workgroup) runs two workgroups, the second partial,
    whose counts meet in the global histogram."""
    img = _own(golden_inputs, "noise_2304")
    want = _policy_a(itw, gpu, oracle, "bc7", "noise_2304", img, "ultrafast", "veryfast", k)
    assert 0 < want["listed"] <= k


@pytest.mark.parametrize("k", [8, 16, 24])
def test_ties_across_the_rank(itw, gpu, oracle, golden_inputs, k):
    """One 16 x 16 patch tiled to 64 x 64: every error value occurs 16 (or a multiple of 16) times.  A group that straddles the rank is
    left off the list as a whole: the listed count is the largest whole number of groups <= k."""
    img = _own(golden_inputs, "tiled")
    ea = R.tier(oracle, "bc7", "tiled", img, "veryfast", 7)[1]
    values, counts = np.unique(ea, return_counts=True)
    assert (counts % 16 == 0).all()
    s = np.sort(ea)[::-1]
    assert s[7] == s[8] and s[23] == s[24]                       # a group straddles ranks 8 and 24
    sizes = counts[::-1]                                         # group sizes, largest error first
    whole = 0
    for n in sizes:
        if whole + n > k:
            break
        whole += n
    want = _policy_a(itw, gpu, oracle, "bc7", "tiled", img, "veryfast", "slow", k)
    assert want["listed"] == whole and whole % 16 == 0
    assert want["budget"][0] == int(s[k])


@pytest.mark.parametrize("k", [0, 1, 256, U])
def test_all_errors_zero(itw, gpu, oracle, golden_inputs, k):
    """A solid colour the first tier encodes exactly: every pass of the select lies above the largest error, T = 0, nothing listed."""
    img = _own(golden_inputs, "solid")
    ea = R.tier(oracle, "bc7", "solid", img, "veryfast", 7)[1]
    assert not ea.any()
    want = _policy_a(itw, gpu, oracle, "bc7", "solid", img, "veryfast", "slow", k)
    assert want["budget"][0] == 0 and want["listed"] == 0 and want["sse_final"] == 0


@pytest.mark.parametrize("k", [0, 1, 15, 16, 17, 128, 255, 256])
def test_wide_keys(itw, gpu, oracle, golden_inputs, k):
    """BC6H fast -> slow on random half codes, all four channels counted (the decoders' alpha of 0x3C00 against random alpha puts the errors
    past 2^33, which the RGB channels alone do not reach under `fast`): four 11-bit digit passes, each of which has to choose between
    digits.  16 errors have the top pass's digit 1: ranks 15 and 16 are its two sides."""
    img = _own(golden_inputs, "half_noise")
    ea = R.tier(oracle, "bc6h", "half_noise", img, "fast", 15)[1]
    assert (ea >= 2 ** 32).any() and ea.max() < 2 ** 39
    assert (ea >= 2 ** 33).sum() == 16
    hi, lo = ea >> 32, ea & (2 ** 32 - 1)
    assert any(np.unique(lo[hi == h]).size > 1 for h in np.unique(hi))       # two errors that differ below bit 32 only
    assert np.unique(hi).size > 1                                            # ... and two that differ above it
    for p in range(4):                                                       # every digit the select scans takes several values
        assert np.unique((ea >> (11 * p)) & 2047).size > 1, p
    want = _policy_a(itw, gpu, oracle, "bc6h", "half_noise", img, "fast", "slow", k, mask=15)
    assert want["budget"][0] == T.select(ea, k)
    if 0 < k < 256:
        assert want["budget"][0] >= 2 ** 22                                  # beyond what two passes hold


def _sse_after(oracle, fmt, key, img, first, refine, rounds):
    """The simulated summed error after `rounds` rounds of an unreachable target."""
    a, ea = R.tier(oracle, fmt, key, img, first, 7)
    b, eb = R.tier(oracle, fmt, key, img, refine, 7)
    cur, tier = ea.copy(), np.zeros(ea.size, dtype=np.uint8)
    for j in range(rounds):
        cand = tier == 0
        t = T.select(cur[cand], T.quota(ea.size, j))
        listed = cand & (cur > t)
        tier[listed] = 1
        cur = np.where(listed & (eb < ea), eb, cur)
    return int(cur.sum())


def test_policy_b_target_already_met(itw, gpu, oracle, golden_inputs):
    img = _img(golden_inputs, "photo")
    a, ea = R.tier(oracle, "bc7", "photo", img, "veryfast", 7)
    for target in (int(ea.sum()), int(ea.sum()) + 1, U - 1):
        want = T.predict(oracle, "bc7", "photo", img, "veryfast", "slow", 7, target=target)
        assert want["rounds"] == 0 and want["target_met"] == 1 and want["listed"] == 0
        got = _run(itw, gpu, "bc7", img, "veryfast", "slow", target_sse=target)
        T.same(got, want, target)
        assert np.array_equal(got[0].cpu().numpy().reshape(-1, 16), a)


def test_policy_b_ends_when_the_target_is_met(itw, gpu, oracle, golden_inputs):
    """The target is the simulated error after two rounds (j = 0, 1): round 0 alone does not reach it, so the call ends after exactly 2."""
    img = _img(golden_inputs, "photo")
    s1, s2 = (_sse_after(oracle, "bc7", "photo", img, "veryfast", "slow", n) for n in (1, 2))
    assert s2 < s1
    want = T.predict(oracle, "bc7", "photo", img, "veryfast", "slow", 7, target=s2)
    assert want["rounds"] == 2 and want["target_met"] == 1 and want["sse_final"] == s2 and all(want["listed_per_round"][:2])
    T.same(_run(itw, gpu, "bc7", img, "veryfast", "slow", target_sse=s2), want, "two rounds")
    want = T.predict(oracle, "bc7", "photo", img, "veryfast", "slow", 7, target=s2 - 1)      # one short: a third round
    assert want["rounds"] >= 3
    T.same(_run(itw, gpu, "bc7", img, "veryfast", "slow", target_sse=s2 - 1), want, "one short of two rounds")


def test_policy_b_unreachable_target(itw, gpu, oracle, golden_inputs):
    img = _img(golden_inputs, "photo")
    ea = R.tier(oracle, "bc7", "photo", img, "veryfast", 7)[1]
    want = T.predict(oracle, "bc7", "photo", img, "veryfast", "slow", 7, target=0)
    assert want["rounds"] == 5 and want["target_met"] == 0 and want["sse_final"] > 0
    assert want["listed"] == int((ea > 0).sum()) == sum(want["listed_per_round"])
    assert want["budget"][4] == 0 and all(b > 0 for b in want["budget"][:4])
    got = _run(itw, gpu, "bc7", img, "veryfast", "slow", target_sse=0)
    T.same(got, want, "target 0")
    assert np.array_equal(got[3].cpu().numpy() > 0, ea > 0)      # every inexact block listed, once


def test_policy_b_cap_ends_a_run_in_mid_round(itw, gpu, oracle, golden_inputs):
    """max_listed 40 of 256 blocks, target 0: round 0 takes its 16, round 1 the 24 that are left of its 32, and the call ends there."""
    img = _img(golden_inputs, "photo")
    want = T.predict(oracle, "bc7", "photo", img, "veryfast", "slow", 7, max_listed=40, target=0)
    assert want["listed_per_round"] == [16, 24, 0, 0, 0] and want["rounds"] == 2 and want["target_met"] == 0
    T.same(_run(itw, gpu, "bc7", img, "veryfast", "slow", max_listed=40, target_sse=0), want, "cap 40")
    want = T.predict(oracle, "bc7", "photo", img, "veryfast", "slow", 7, max_listed=0, target=0)
    assert want["rounds"] == 0
    T.same(_run(itw, gpu, "bc7", img, "veryfast", "slow", max_listed=0, target_sse=0), want, "cap 0")


def test_policy_b_an_empty_round_falls_through(itw, gpu, oracle, golden_inputs):
    """The tiled image with the patch's worst block copied over its neighbour: the largest error occurs 32 times, round 0's rank of 16
    falls inside that group and lists nothing, round 1's rank of 32 takes it."""
    key = "tiled_top32"
    if key not in _content:
        patch = np.array(_own(golden_inputs, "tiled")[:16, :16])
        e = R.block_errors(oracle, "bc7", oracle.encode("bc7", patch, "veryfast"), patch, 7)
        y, x = divmod(int(e.argmax()), 4)
        x2 = (x + 1) % 4
        patch[4 * y:4 * y + 4, 4 * x2:4 * x2 + 4] = patch[4 * y:4 * y + 4, 4 * x:4 * x + 4]
        img = np.ascontiguousarray(np.tile(patch, (4, 4, 1)))
        img.setflags(write=False)
        _content[key] = img
    img = _content[key]
    ea = R.tier(oracle, "bc7", key, img, "veryfast", 7)[1]
    assert (ea == ea.max()).sum() == 32
    want = T.predict(oracle, "bc7", key, img, "veryfast", "slow", 7, target=0)
    assert want["listed_per_round"][0] == 0 and want["listed_per_round"][1] == 32 and want["rounds"] == 5
    assert want["budget"][0] == int(ea.max())
    T.same(_run(itw, gpu, "bc7", img, "veryfast", "slow", target_sse=0), want, "empty round 0")


def test_policy_b_bc6h(itw, gpu, oracle, golden_inputs):
    img = _img(golden_inputs, "hdr")
    s2 = _sse_after(oracle, "bc6h", "hdr", img, "veryfast", "slow", 2)
    want = T.predict(oracle, "bc6h", "hdr", img, "veryfast", "slow", 7, target=s2)
    assert want["rounds"] == 2 and want["target_met"] == 1 and 0 < want["replaced"]
    T.same(_run(itw, gpu, "bc6h", img, "veryfast", "slow", target_sse=s2), want, "bc6h, two rounds")
    want = T.predict(oracle, "bc6h", "hdr", img, "veryfast", "slow", 7, max_listed=100, target=0)
    assert want["listed"] == 100 and want["target_met"] == 0
    T.same(_run(itw, gpu, "bc6h", img, "veryfast", "slow", max_listed=100, target_sse=0), want, "bc6h, cap 100")


def test_same_bits_on_two_runs(itw, gpu, golden_inputs):
    import torch
    for fmt, key, first, refine, policy in (("bc7", "noise_576", "ultrafast", "veryfast", {"max_listed": 200}),
                                            ("bc7", "photo", "veryfast", "slow", {"target_sse": 0}),
                                            ("bc6h", "hdr", "veryfast", "slow", {"max_listed": 90, "target_sse": 0})):
        img = _img(golden_inputs, key)
        one = _run(itw, gpu, fmt, img, first, refine, **policy)
        two = _run(itw, gpu, fmt, img, first, refine, **policy)
        assert bytes(one[1]) == bytes(two[1]), (fmt, key)
        for x, y in zip((one[0], one[2], one[3]), (two[0], two[2], two[3])):
            assert torch.equal(x, y), (fmt, key)


def test_pointer_kinds(itw, gpu, oracle, golden_inputs):
    """All host pointers through the binding, and all device pointers (stats too) through the C call: the same bytes."""
    import torch
    img = _img(golden_inputs, "noise_576")
    want = T.predict(oracle, "bc7", "noise_576", img, "ultrafast", "veryfast", 7, max_listed=100)
    T.same(itw.compress_refined_to("bc7", img, "ultrafast", "veryfast", max_listed=100, want_block_map=True, want_tier_map=True), want, "all host")
    itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
    src = R.to_gpu(gpu, img)
    out = torch.zeros(576 * 16, dtype=torch.uint8, device=gpu)
    stats = torch.zeros(C.sizeof(itw.RefineTargetStats), dtype=torch.uint8, device=gpu)
    bmap = torch.zeros(576, dtype=torch.int64, device=gpu)
    tmap = torch.full((576,), 9, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    s1, s2, pol = itw.bc7_profile("ultrafast"), itw.bc7_profile("veryfast"), itw.RefinePolicy(100, U)
    surf = itw.RgbaSurface(src.data_ptr(), 128, 72, 128 * 4)
    ok = itw.lib().itwCompressImageRefinedTo(C.byref(surf), out.data_ptr(), 98, C.addressof(s1), C.addressof(s2), 7, C.addressof(pol), C.sizeof(pol),
                                             stats.data_ptr(), C.sizeof(itw.RefineTargetStats), bmap.data_ptr(), tmap.data_ptr())
    assert ok, itw.last_error()
    T.same((out, itw.RefineTargetStats.from_buffer_copy(stats.cpu().numpy().tobytes()), bmap, tmap), want, "all device")


def test_python_share_and_target_psnr(itw, gpu, oracle, golden_inputs):
    """share= is max_listed = floor(share * blocks); target_psnr= is target_sse = itwPsnrToTotalSse(...): the same calls."""
    import torch
    img = _img(golden_inputs, "photo")
    dev = R.to_gpu(gpu, img)

    def call(**policy):
        got = itw.compress_refined_to("bc7", dev, "veryfast", "slow", want_block_map=True, want_tier_map=True, **policy)
        torch.cuda.synchronize()
        return got

    def equal(one, two):
        return bytes(one[1]) == bytes(two[1]) and all(torch.equal(x, y) for x, y in zip((one[0], one[2], one[3]), (two[0], two[2], two[3])))

    by_share = call(share=0.3)
    assert equal(by_share, call(max_listed=76))                  # floor(0.3 * 256)
    T.same(by_share, T.predict(oracle, "bc7", "photo", img, "veryfast", "slow", 7, max_listed=76), "share 0.3")
    ea = R.tier(oracle, "bc7", "photo", img, "veryfast", 7)[1]
    eb = R.tier(oracle, "bc7", "photo", img, "slow", 7)[1]
    first_db, best_db = (10.0 * np.log10(255.0 ** 2 * 64 * 64 * 3 / float(e.sum())) for e in (ea, np.minimum(ea, eb)))
    db = 0.5 * (first_db + best_db)                              # between what the first tier gives and the best the two can give
    target = itw.psnr_to_total_sse("bc7", 64, 64, db)
    assert target == itw.lib().itwPsnrToTotalSse(98, 64, 64, 7, db) and int(np.minimum(ea, eb).sum()) < target < int(ea.sum())
    by_psnr = call(target_psnr=db)
    assert equal(by_psnr, call(target_sse=target))
    want = T.predict(oracle, "bc7", "photo", img, "veryfast", "slow", 7, target=target)
    assert want["rounds"] >= 1 and want["target_met"] == 1
    T.same(by_psnr, want, "target_psnr")
    for bad in ({"share": 0.3, "max_listed": 5}, {"target_psnr": 40.0, "target_sse": 5}, {"share": 1.5}):
        with pytest.raises(ValueError):
            itw.compress_refined_to("bc7", dev, "veryfast", "slow", **bad)
    with pytest.raises(ValueError):
        itw.compress_refined_to("bc6h", R.to_gpu(gpu, _img(golden_inputs, "hdr")), "veryfast", "slow", target_psnr=40.0)


def test_example_refine_share_option(itw, oracle, gpu, tmp_path):
    """examples/encode_dds --refine-share <profile> <percent>: the .dds payload is what the binding returns for share = percent / 100."""
    import os
    import subprocess
    from itw_amd import surfaces
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "encode_dds")
    img = surfaces.ldr_smooth(64, 64)
    want = T.predict(oracle, "bc7", "ldr_smooth_64", img, "veryfast", "slow", 7, max_listed=64)
    assert 0 < want["replaced"] and 0 < want["listed"] <= 64
    raw, dds = tmp_path / "in.raw", tmp_path / "out.dds"
    img.tofile(raw)
    r = subprocess.run([exe, "--refine-share", "slow", "25", "bc7_veryfast", "64", "64", str(raw), str(dds)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    payload = np.fromfile(dds, dtype=np.uint8)[-256 * 16:]
    got = itw.compress_refined_to("bc7", img, "veryfast", "slow", share=0.25)
    assert np.array_equal(payload, got[0])
    assert np.array_equal(payload.reshape(-1, 16), want["target"])
    assert r.stdout.strip() == ("refined: bc7_veryfast -> slow share 25 rounds 1 met 1 budgets [{b}, 0, 0, 0, 0] blocks {blocks} listed {listed} replaced {replaced} "
                                "sse {sse_first} -> {sse_final} worst {worst_first} -> {worst_final}").format(b=want["budget"][0], **want)
