"""WHERE itwCompressImageRefined writes: device target, stats, block_sse and tier_map each between guard bands of the fill pattern
(tests/_guarded.py), the source frozen, in the manner of tests/test_gpu_write_extents.py.  With nothing, one block and every block
listed: the payloads equal the oracle's prediction -- so every byte inside was written, none of them still the pattern's -- and the
bands are intact, on two consecutive calls into re-patterned buffers."""
import ctypes as C

import numpy as np
import pytest

import _refine as R
from _guarded import frozen, guarded

pytestmark = pytest.mark.gpu

W, H, N = 68, 60, 17 * 15                                        # 255 blocks: one short of a workgroup, and of a packed row


@pytest.mark.parametrize("count", [0, 1, N])
def test_outputs_stay_inside_their_buffers(itw, gpu, oracle, count):
    import torch
    img = np.random.default_rng(68).integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    ea = R.tier(oracle, "bc7", "noise_68x60", img, "ultrafast", 7)[1]
    s = np.sort(ea)
    assert s[0] > 0 and s[-2] < s[-1]
    budget = {0: int(s[-1]), 1: int(s[-2]), N: 0}[count]
    want = R.predict(oracle, "bc7", "noise_68x60", img, "ultrafast", "veryfast", 7, budget)
    assert want["listed"] == count

    src = frozen(img, row_pad=48, device=gpu)
    out, stats, bmap, tmap = (guarded(N * 16, device=gpu), guarded(C.sizeof(itw.RefineStats), device=gpu), guarded(N * 8, device=gpu),
                              guarded(N, device=gpu))
    s1, s2 = itw.bc7_profile("ultrafast"), itw.bc7_profile("veryfast")
    surf = itw.RgbaSurface(src.ptr, W, H, src.stride)
    itw.lib().itwSetStream(torch.cuda.current_stream(gpu).cuda_stream)
    for rnd in (1, 2):
        for o in (out, stats, bmap, tmap):
            o.refill()
        ok = itw.lib().itwCompressImageRefined(C.byref(surf), out.ptr, 98, C.addressof(s1), C.addressof(s2), 7, budget, stats.ptr,
                                               C.sizeof(itw.RefineStats), bmap.ptr, tmap.ptr)
        assert ok, itw.last_error()
        torch.cuda.synchronize()
        got = (out.host(), itw.RefineStats.from_buffer_copy(stats.host().tobytes()), bmap.host().view(np.uint64), tmap.host())
        R.same(got, want, (count, f"call {rnd}"))
        for name, o in (("target", out), ("stats", stats), ("block_sse", bmap), ("tier_map", tmap)):
            o.check(f"{count} listed, call {rnd}, {name}")
        src.check(f"{count} listed, call {rnd}, source")
