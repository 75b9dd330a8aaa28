"""itwCompressImageChainRefined / itwCompressImageChainRefinedTo against the CPU oracle's prediction (tests/_refine_chain.py): every
output and every stats field, whole-chain and per image, compared with ==.

The content is the ODD CHAIN: seeded uniform noise (RGBA8, or 16-bit patterns below 0x7BFF for BC6H) at ten sizes that make 1135 blocks
-- a second packed row behind block 1024, several image boundaries inside one wave, three one-block images and every partial extent
pw, ph in {1, 2, 3, 4}.  What the tests rely on is asserted on the CPU side before any call (test_the_odd_chain_is_what_the_tests_need):
for seed 53 the cropped and the uncropped error differ in 54 (BC7) / 55 (BC6H) blocks, the median budget lists 567 blocks of which
ultrafast -> veryfast replaces 567, alpha_veryfast -> alpha_slow 379 (per image some win and some lose) and BC6H veryfast -> slow 561,
the first tier leaves exactly one exact block, and no two errors are equal across the ranks the list-edge tests cut at."""
import numpy as np
import pytest

import _refine as R
import _refine_chain as RC
import _refine_target as T

pytestmark = pytest.mark.gpu

SEED = 53
SIZES = [(132, 100), (66, 50), (33, 25), (16, 12), (8, 6), (4, 3), (2, 1), (1, 1), (7, 5), (3, 11)]       # (w, h)
STARTS = [0, 825, 1046, 1109, 1121, 1125, 1126, 1127, 1128, 1132]
N = 1135
RANKS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1134)
CASES = [("bc7", "ultrafast", "veryfast", 7), ("bc7", "alpha_veryfast", "alpha_slow", 15), ("bc6h", "veryfast", "slow", 7)]
CHANNELS = {7: "rgb", 15: "rgba"}
_chains = {}


def noise(fmt, rng, w, h):
    if fmt == "bc6h":
        return rng.integers(0, 0x7BFF, size=(h, w, 4), dtype=np.uint16)
    return rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)


def odd_chain(fmt):
    """(key, images): computed once per format and frozen."""
    if fmt not in _chains:
        rng = np.random.default_rng(SEED)
        images = [noise(fmt, rng, w, h) for w, h in SIZES]
        for im in images:
            im.setflags(write=False)
        _chains[fmt] = (f"odd_chain_{SEED}", images)
    return _chains[fmt]


def call(itw, gpu, fmt, images, first, refine, budget, mask, where):
    src = [R.to_gpu(gpu, im) for im in images] if where == "device" else images
    return itw.compress_chain_refined(fmt, src, first, refine, budget, channels=CHANNELS[mask], want_block_map=True, want_tier_map=True,
                                      want_image_stats=True)


def call_to(itw, gpu, fmt, images, first, refine, mask, where="device", **policy):
    src = [R.to_gpu(gpu, im) for im in images] if where == "device" else images
    return itw.compress_chain_refined_to(fmt, src, first, refine, channels=CHANNELS[mask], want_block_map=True, want_tier_map=True,
                                         want_image_stats=True, **policy)


def median_budget(oracle, fmt, key, images, first, mask):
    return int(np.sort(RC.tier(oracle, fmt, key, images, first, mask)[1])[N // 2])


@pytest.mark.parametrize("fmt,first,refine,mask", CASES)
def test_the_odd_chain_is_what_the_tests_need(oracle, fmt, first, refine, mask):
    key, images = odd_chain(fmt)
    starts, n = RC.starts(images)
    assert (starts, n) == (STARTS, N)
    assert {min(4, w - x) for w, _ in SIZES for x in range(0, w, 4)} == {min(4, h - y) for _, h in SIZES for y in range(0, h, 4)} == {1, 2, 3, 4}
    _, ea, full = RC.tier(oracle, fmt, key, images, first, mask)
    _, eb, full_b = RC.tier(oracle, fmt, key, images, refine, mask)
    assert int((ea != full).sum()) == (55 if fmt == "bc6h" else 54)
    s = np.sort(ea)[::-1]
    assert not [k for k in RANKS + (N // 2, N // 2 + 1) if s[k - 1] == s[k]]
    want = RC.predict(oracle, fmt, key, images, first, refine, mask, median_budget(oracle, fmt, key, images, first, mask))
    # padding is not counted: counting it would change at least one block of the predicted map in every image that has a partial block
    counted = np.where(want["tier_map"] == 2, full_b, full)
    for (w, h), a, b in zip(SIZES, STARTS, STARTS[1:] + [N]):
        assert (want["block_sse"][a:b] != counted[a:b]).any() == bool(w % 4 or h % 4), (w, h)
    assert want["listed"] == 567
    assert want["replaced"] == {"veryfast": 567, "alpha_slow": 379, "slow": 561}[refine]
    if refine == "alpha_slow":                                    # per image some win and some lose
        assert sum(1 for i in want["image_stats"] if 0 < i["replaced"] < i["listed"]) >= 3
    if first == "ultrafast":
        assert int((ea == 0).sum()) == 1                          # the one exact block of the list-edge tests


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("fmt,first,refine,mask", CASES)
def test_parity_with_the_oracle(itw, gpu, oracle, fmt, first, refine, mask, where):
    key, images = odd_chain(fmt)
    budget = median_budget(oracle, fmt, key, images, first, mask)
    want = RC.predict(oracle, fmt, key, images, first, refine, mask, budget)
    RC.same(call(itw, gpu, fmt, images, first, refine, budget, mask, where), want, (fmt, first, refine, where))


@pytest.mark.parametrize("fmt,first,refine,mask", CASES)
def test_padding_is_not_counted(itw, gpu, oracle, fmt, first, refine, mask):
    """What the call reports per image is what itwMeasureChain measures of the stream it wrote: the texels inside the image."""
    key, images = odd_chain(fmt)
    budget = median_budget(oracle, fmt, key, images, first, mask)
    src = [R.to_gpu(gpu, im) for im in images]
    got = itw.compress_chain_refined(fmt, src, first, refine, budget, channels=CHANNELS[mask], want_image_stats=True)
    measured = itw.measure_chain(fmt, got[0], src)
    for i, (st, per) in enumerate(zip(measured, got[2])):
        assert sum(int(st.sse[c]) for c in range(4) if mask >> c & 1) == int(per.sse_final), (i, SIZES[i])
    assert sum(int(p.sse_final) for p in got[2]) == int(got[1].sse_final)


@pytest.mark.parametrize("count", (0,) + RANKS)
def test_list_edges(itw, gpu, oracle, count):
    """Exactly `count` blocks listed: an empty list, one block, one less than / exactly / one more than a wave, a workgroup (and a packed
    row of the refine tier's surface) and the chain's first packed row, and all but the one exact block."""
    fmt, first, refine, mask = CASES[0]
    key, images = odd_chain(fmt)
    s = np.sort(RC.tier(oracle, fmt, key, images, first, mask)[1])[::-1]
    budget = int(s[count])
    want = RC.predict(oracle, fmt, key, images, first, refine, mask, budget)
    assert want["listed"] == count
    RC.same(call(itw, gpu, fmt, images, first, refine, budget, mask, "device"), want, count)


def test_budget_0_lists_every_block_that_is_not_exact(itw, gpu, oracle):
    fmt, first, refine, mask = CASES[0]
    key, images = odd_chain(fmt)
    want = RC.predict(oracle, fmt, key, images, first, refine, mask, 0)
    assert want["listed"] == N - 1
    assert want["image_stats"][5]["listed"] == 1 and want["image_stats"][6]["listed"] == 1      # the 4 x 3 and the 2 x 1 image with it
    RC.same(call(itw, gpu, fmt, images, first, refine, 0, mask, "device"), want, "budget 0")


@pytest.mark.parametrize("fmt,first,refine,mask", CASES)
def test_cube_with_mips(itw, gpu, oracle, fmt, first, refine, mask):
    """Six faces x levels 16, 8, 4, 2, 1 in DDS order: 138 blocks, 18 of them one-texel-wide or -high tail mips."""
    rng = np.random.default_rng(6)
    images = [noise(fmt, rng, s, s) for _ in range(6) for s in (16, 8, 4, 2, 1)]
    key = "cube_16"
    assert RC.starts(images)[1] == 138
    ea = RC.tier(oracle, fmt, key, images, first, mask)[1]
    budget = int(np.sort(ea)[69])
    want = RC.predict(oracle, fmt, key, images, first, refine, mask, budget)
    assert 0 < want["listed"] < 138
    RC.same(call(itw, gpu, fmt, images, first, refine, budget, mask, "device"), want, "cube")
    # nothing listed: the plain chain encode under the first preset, byte for byte
    nothing = RC.predict(oracle, fmt, key, images, first, refine, mask, R.U64_MAX)
    got = call(itw, gpu, fmt, images, first, refine, R.U64_MAX, mask, "device")
    RC.same(got, nothing, "cube, nothing listed")
    ok, plain = itw.compress_chain(fmt, [R.to_gpu(gpu, im) for im in images], first)
    assert ok and np.array_equal(got[0].cpu().numpy(), plain.cpu().numpy())


@pytest.mark.parametrize("fmt,first,refine,mask", CASES)
def test_a_chain_of_one_image_is_the_single_image_call(itw, gpu, oracle, fmt, first, refine, mask):
    img = noise(fmt, np.random.default_rng(64), 64, 64)
    key = "noise_64"
    ea = RC.tier(oracle, fmt, key, [img], first, mask)[1]
    budget = int(np.sort(ea)[128])
    want = RC.predict(oracle, fmt, key, [img], first, refine, mask, budget)
    chain = call(itw, gpu, fmt, [img], first, refine, budget, mask, "device")
    RC.same(chain, want, "chain of one")
    single = itw.compress_refined(fmt, R.to_gpu(gpu, img), first, refine, budget, channels=CHANNELS[mask], want_block_map=True, want_tier_map=True)
    for a, b in zip((chain[0], chain[2], chain[3]), (single[0], single[2], single[3])):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert chain[1].as_dict() == single[1].as_dict() == chain[4][0].as_dict()
    for policy in ({"max_listed": 100}, {"target_sse": (int(ea.sum()) * 3) // 4}):
        want = RC.predict_to(oracle, fmt, key, [img], first, refine, mask, policy.get("max_listed", R.U64_MAX), policy.get("target_sse", R.U64_MAX))
        chain = call_to(itw, gpu, fmt, [img], first, refine, mask, **policy)
        RC.same_to(chain, want, ("chain of one", policy))
        single = itw.compress_refined_to(fmt, R.to_gpu(gpu, img), first, refine, channels=CHANNELS[mask], want_block_map=True, want_tier_map=True, **policy)
        for a, b in zip((chain[0], chain[2], chain[3]), (single[0], single[2], single[3])):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
        assert chain[1].as_dict() == single[1].as_dict()
        assert chain[1].total.as_dict() == chain[4][0].as_dict()


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("fmt,first,refine,mask", [CASES[0], CASES[2]])
def test_views_into_one_canvas(itw, gpu, oracle, fmt, first, refine, mask, where):
    """The odd chain as views into one allocation: strides above the row's bytes, starts that are no multiple of 16 bytes."""
    import torch
    key, images = odd_chain(fmt)
    isz = images[0].itemsize
    px = 4 * isz
    offs, strides, at = [], [], px                                # in bytes; every start is a multiple of a texel, not of 16
    for im in images:
        h, w = im.shape[:2]
        stride = w * px + 16 + px
        if at % 16 == 0:
            at += px
        offs.append(at)
        strides.append(stride)
        at += h * stride + px
    canvas = np.full(at + 64, 0xA5, dtype=np.uint8)
    for im, o, st in zip(images, offs, strides):
        h, w = im.shape[:2]
        np.ndarray((h, w * px), np.uint8, canvas, o, (st, 1))[:] = im.view(np.uint8).reshape(h, w * px)
    assert all(o % 16 for o in offs)
    if where == "host":
        keep = canvas.copy()
        views = [np.ndarray(im.shape, im.dtype, canvas, o, (st, px, isz)) for im, o, st in zip(images, offs, strides)]
    else:
        dev = torch.from_numpy(canvas).to(gpu)
        flat = dev.view(torch.int16) if isz == 2 else dev
        views = [torch.as_strided(flat, im.shape, (st // isz, 4, 1), o // isz) for im, o, st in zip(images, offs, strides)]
    budget = median_budget(oracle, fmt, key, images, first, mask)
    want = RC.predict(oracle, fmt, key, images, first, refine, mask, budget)
    got = itw.compress_chain_refined(fmt, views, first, refine, budget, channels=CHANNELS[mask], want_block_map=True, want_tier_map=True,
                                     want_image_stats=True)
    RC.same(got, want, ("views", where))
    assert np.array_equal(keep if where == "host" else dev.cpu().numpy(), canvas)


@pytest.mark.parametrize("k", (0,) + RANKS)
def test_refined_to_lists_the_k_worst_blocks(itw, gpu, oracle, k):
    """Policy A over the chain as one population: the simulation's outputs, and byte for byte compress_chain_refined with T."""
    fmt, first, refine, mask = CASES[0]
    key, images = odd_chain(fmt)
    want = RC.predict_to(oracle, fmt, key, images, first, refine, mask, max_listed=k)
    assert want["listed"] == k
    got = call_to(itw, gpu, fmt, images, first, refine, mask, max_listed=k)
    RC.same_to(got, want, k)
    fixed = call(itw, gpu, fmt, images, first, refine, int(got[1].budget[0]), mask, "device")
    for a, b in zip((got[0], got[2], got[3]), (fixed[0], fixed[2], fixed[3])):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert got[1].total.as_dict() == fixed[1].as_dict()
    assert [p.as_dict() for p in got[4]] == [p.as_dict() for p in fixed[4]]


def test_refined_to_leaves_a_group_of_equal_errors_off_the_list_whole(itw, gpu, oracle):
    """One 8 x 8 image three times in the chain: each of its four errors occurs three times; k falls inside the worst such group."""
    fmt, first, refine, mask = CASES[0]
    rng = np.random.default_rng(88)
    twin = noise(fmt, rng, 8, 8)
    images = [noise(fmt, rng, 16, 12), twin, noise(fmt, rng, 7, 5), twin, noise(fmt, rng, 3, 11), twin]
    key = "twins_88"
    ea = RC.tier(oracle, fmt, key, images, first, mask)[1]
    starts, n = RC.starts(images)
    v = int(ea[starts[1]:starts[1] + 4].max())
    above = int((ea > v).sum())
    assert int((ea == v).sum()) == 3 and above > 0
    for k in (above + 1, above + 2):                              # inside the group: it stays off the list whole
        want = RC.predict_to(oracle, fmt, key, images, first, refine, mask, max_listed=k)
        assert want["listed"] == above and want["budget"][0] == v
        RC.same_to(call_to(itw, gpu, fmt, images, first, refine, mask, max_listed=k), want, k)
    want = RC.predict_to(oracle, fmt, key, images, first, refine, mask, max_listed=above + 3)
    assert want["listed"] == above + 3
    RC.same_to(call_to(itw, gpu, fmt, images, first, refine, mask, max_listed=above + 3), want, above + 3)


@pytest.mark.parametrize("fmt,first,refine,mask", CASES)
def test_refined_to_reaches_a_summed_error(itw, gpu, oracle, fmt, first, refine, mask):
    """Policy B: targets a third and two thirds of the way from the first preset's summed error to the refine preset's, and a target
    nothing reaches under a cap of 300 blocks; rounds, budget[], listed[] and target_met against the simulation."""
    key, images = odd_chain(fmt)
    sa = int(RC.tier(oracle, fmt, key, images, first, mask)[1].sum())
    sb = int(RC.tier(oracle, fmt, key, images, refine, mask)[1].sum())
    assert sb < sa
    for target in (sa - (sa - sb) // 3, sa - 2 * (sa - sb) // 3):
        want = RC.predict_to(oracle, fmt, key, images, first, refine, mask, target=target)
        assert want["target_met"] == 1 and 1 <= want["rounds"] <= 5
        RC.same_to(call_to(itw, gpu, fmt, images, first, refine, mask, target_sse=target), want, target)
    want = RC.predict_to(oracle, fmt, key, images, first, refine, mask, max_listed=300, target=0)
    assert want["target_met"] == 0 and want["listed"] <= 300
    RC.same_to(call_to(itw, gpu, fmt, images, first, refine, mask, max_listed=300, target_sse=0), want, "unreachable")


@pytest.mark.parametrize("first,refine,mask", [CASES[0][1:], CASES[1][1:]])
def test_refined_to_reaches_a_psnr_over_the_chain(itw, gpu, oracle, first, refine, mask):
    import math
    fmt = "bc7"
    key, images = odd_chain(fmt)
    sa = int(RC.tier(oracle, fmt, key, images, first, mask)[1].sum())
    sb = int(RC.tier(oracle, fmt, key, images, refine, mask)[1].sum())
    n = sum(w * h for w, h in SIZES) * bin(mask).count("1")
    db = 10.0 * math.log10(255.0 * 255.0 * n / ((sa + sb) / 2.0))
    target = itw.chain_psnr_to_total_sse(fmt, images, db, CHANNELS[mask])
    assert abs(target - (sa + sb) // 2) <= 1
    want = RC.predict_to(oracle, fmt, key, images, first, refine, mask, target=target)
    assert want["target_met"] == 1
    got = call_to(itw, gpu, fmt, images, first, refine, mask, target_psnr=db)
    RC.same_to(got, want, db)
    assert 10.0 * math.log10(255.0 * 255.0 * n / int(got[1].total.sse_final)) >= db
