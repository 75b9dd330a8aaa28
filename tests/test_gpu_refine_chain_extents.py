"""WHERE itwCompressImageChainRefined[To] write: target (itwChainBytes), stats, image_stats (count entries), block_sse (n) and tier_map (n)
each between guard bands of the fill pattern (tests/_guarded.py), the source images frozen, in the manner of
tests/test_gpu_refine_extents.py.  Device and host outputs, with and without the optional ones; the payloads equal the oracle's
prediction -- so every byte inside was written -- and the bands are intact, on two consecutive calls into re-patterned buffers.

The chain: 20 x 12, 9 x 7, 4 x 4, 2 x 3, 1 x 1 noise: 24 blocks -- the first tier's packed surface is 24 blocks wide and one block row
high, so its encoding fills exactly n blocks of scratch -- and a second chain of 1030 blocks whose packed surface has a second row of
which 1018 blocks are tail: what the first tier writes past n must stay in scratch."""
import ctypes as C

import numpy as np
import pytest

import _refine as R
import _refine_chain as RC
from _guarded import frozen, guarded

pytestmark = pytest.mark.gpu

CHAINS = {"small": [(20, 12), (9, 7), (4, 4), (2, 3), (1, 1)], "two_rows": [(128, 128), (9, 7)]}      # (w, h)


def _chain(name):
    rng = np.random.default_rng(len(name))
    return [rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8) for w, h in CHAINS[name]]


@pytest.mark.parametrize("optional", [True, False])
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("entry", ["budget", "to"])
@pytest.mark.parametrize("name", ["small", "two_rows"])
def test_outputs_stay_inside_their_buffers(itw, gpu, oracle, name, entry, where, optional):
    import torch
    images = _chain(name)
    key = "extents_" + name
    count = len(images)
    n = RC.starts(images)[1]
    assert n == {"small": 24, "two_rows": 1030}[name] and itw.chain_bytes("bc7", images) == n * 16
    ea = RC.tier(oracle, "bc7", key, images, "ultrafast", 7)[1]
    s = np.sort(ea)[::-1]
    k = n // 3
    assert s[k - 1] > s[k]
    if entry == "budget":
        want = RC.predict(oracle, "bc7", key, images, "ultrafast", "veryfast", 7, int(s[k]))
        stats_type = itw.RefineStats
    else:
        want = RC.predict_to(oracle, "bc7", key, images, "ultrafast", "veryfast", 7, max_listed=k)
        stats_type = itw.RefineTargetStats
    assert want["listed"] == k

    dev = gpu if where == "device" else None
    srcs = [frozen(im, row_pad=20, device=gpu, offset=4) for im in images]
    out, stats = guarded(n * 16, device=dev), guarded(C.sizeof(stats_type), device=dev)
    per, bmap, tmap = guarded(count * C.sizeof(itw.RefineStats), device=dev), guarded(n * 8, device=dev), guarded(n, device=dev)
    s1, s2 = itw.bc7_profile("ultrafast"), itw.bc7_profile("veryfast")
    pol = itw.RefinePolicy(k, R.U64_MAX)
    surfs = (itw.RgbaSurface * count)(*[itw.RgbaSurface(f.ptr, im.shape[1], im.shape[0], f.stride) for f, im in zip(srcs, images)])
    L = itw.lib()
    L.itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
    opt = (per.ptr, bmap.ptr, tmap.ptr) if optional else (None, None, None)
    for rnd in (1, 2):
        for o in (out, stats, per, bmap, tmap):
            o.refill()
        if entry == "budget":
            ok = L.itwCompressImageChainRefined(C.cast(surfs, C.c_void_p), count, out.ptr, 98, C.addressof(s1), C.addressof(s2), 7, int(s[k]), stats.ptr,
                                                C.sizeof(stats_type), *opt)
        else:
            ok = L.itwCompressImageChainRefinedTo(C.cast(surfs, C.c_void_p), count, out.ptr, 98, C.addressof(s1), C.addressof(s2), 7, C.addressof(pol),
                                                  C.sizeof(pol), stats.ptr, C.sizeof(stats_type), *opt)
        assert ok, itw.last_error()
        torch.cuda.synchronize()
        what = (name, entry, where, optional, f"call {rnd}")
        st = stats_type.from_buffer_copy(stats.host().tobytes())
        if optional:
            each = [itw.RefineStats.from_buffer_copy(per.host()[i * 56:(i + 1) * 56].tobytes()) for i in range(count)]
            got = (out.host(), st, bmap.host().view(np.uint64), tmap.host(), each)
            (RC.same if entry == "budget" else RC.same_to)(got, want, what)
        else:
            assert np.array_equal(out.host().reshape(-1, 16), want["target"]), what
            total = st.as_dict() if entry == "budget" else st.total.as_dict()
            assert all(total[f] == want[f] for f in R.STATS), what
            for o in (per, bmap, tmap):                           # not passed: not touched, payload included
                assert np.array_equal(o._whole(), o._expect), what
        for label, o in (("target", out), ("stats", stats), ("image_stats", per), ("block_sse", bmap), ("tier_map", tmap)):
            o.check(f"{what}, {label}")
        for i, f in enumerate(srcs):
            f.check(f"{what}, image {i}")
