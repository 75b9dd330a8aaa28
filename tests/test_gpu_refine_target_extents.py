"""WHERE itwCompressImageRefinedTo writes: device target, stats, block_sse and tier_map each between guard bands of the fill pattern
(tests/_guarded.py), the source frozen, in the manner of tests/test_gpu_refine_extents.py.  Policy A with nothing, one block and every
block listed, and policy B over all five rounds: the payloads equal the oracle's prediction -- so every byte inside was written, none of
them still the pattern's -- and the bands are intact, on two consecutive calls into re-patterned buffers."""
import ctypes as C

import numpy as np
import pytest

import _refine as R
import _refine_target as T
from _guarded import frozen, guarded

pytestmark = pytest.mark.gpu

W, H, N = 68, 60, 17 * 15                                        # 255 blocks: one short of a workgroup, and of a packed row


@pytest.mark.parametrize("max_listed,target", [(0, T.U64_MAX), (1, T.U64_MAX), (T.U64_MAX, T.U64_MAX), (T.U64_MAX, 0)],
                         ids=["none", "one", "all", "five-rounds"])
def test_outputs_stay_inside_their_buffers(itw, gpu, oracle, max_listed, target):
    import torch
    img = np.random.default_rng(68).integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    ea = R.tier(oracle, "bc7", "noise_68x60", img, "ultrafast", 7)[1]
    s = np.sort(ea)
    assert s[0] > 0 and s[-2] < s[-1]
    want = T.predict(oracle, "bc7", "noise_68x60", img, "ultrafast", "veryfast", 7, max_listed=max_listed, target=target)
    assert want["listed"] == min(max_listed, N) and want["rounds"] == (1 if target == T.U64_MAX else 5)

    src = frozen(img, row_pad=48, device=gpu)
    out, stats, bmap, tmap = (guarded(N * 16, device=gpu), guarded(C.sizeof(itw.RefineTargetStats), device=gpu), guarded(N * 8, device=gpu),
                              guarded(N, device=gpu))
    s1, s2, pol = itw.bc7_profile("ultrafast"), itw.bc7_profile("veryfast"), itw.RefinePolicy(max_listed, target)
    surf = itw.RgbaSurface(src.ptr, W, H, src.stride)
    itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
    for rnd in (1, 2):
        for o in (out, stats, bmap, tmap):
            o.refill()
        ok = itw.lib().itwCompressImageRefinedTo(C.byref(surf), out.ptr, 98, C.addressof(s1), C.addressof(s2), 7, C.addressof(pol), C.sizeof(pol),
                                                 stats.ptr, C.sizeof(itw.RefineTargetStats), bmap.ptr, tmap.ptr)
        assert ok, itw.last_error()
        torch.cuda.synchronize()
        got = (out.host(), itw.RefineTargetStats.from_buffer_copy(stats.host().tobytes()), bmap.host().view(np.uint64), tmap.host())
        T.same(got, want, (max_listed, target, f"call {rnd}"))
        for name, o in (("target", out), ("stats", stats), ("block_sse", bmap), ("tier_map", tmap)):
            o.check(f"{max_listed} / {target}, call {rnd}, {name}")
        src.check(f"{max_listed} / {target}, call {rnd}, source")
