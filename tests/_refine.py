"""What itwCompressImageRefined has to return, predicted by the CPU oracle alone (tests/test_gpu_refine.py, test_gpu_refine_extents.py).

A = oracle.encode(first), B = oracle.encode(refine), both over the whole image (blocks are independent); the per-block errors of both from
oracle.decode in numpy int64, as tests/test_gpu_measure.py::_expect computes them, summed over the channels of the mask; then the rule of
include/itw_dispatch.h.  Encodings and error maps are computed once per (format, content, preset, mask) and never modified."""
import numpy as np

U64_MAX = 2 ** 64 - 1
STATS = ("blocks", "listed", "replaced", "sse_first", "sse_final", "worst_first", "worst_final")

_cache = {}


def block_errors(oracle, fmt, blocks, img, mask):
    """int64 per-block sums of the squared code differences of the channels in `mask` (bit 0 = R .. bit 3 = A), raster block order."""
    h, w = img.shape[:2]
    dec, _ = oracle.decode(fmt, blocks, w, h)
    if fmt == "bc6h":                                            # the decoders fill alpha with 1.0
        full = np.empty((h, w, 4), dtype=np.uint16)
        full[..., :3] = dec
        full[..., 3] = 0x3C00
        dec = full
    d = img.astype(np.int64) - dec.astype(np.int64)
    sq = (d * d)[..., [c for c in range(4) if mask >> c & 1]].sum(axis=2)
    return sq.reshape(h // 4, 4, w // 4, 4).sum(axis=(1, 3)).reshape(-1)


def tier(oracle, fmt, key, img, prof, mask, mt=False):
    """(blocks as (n, 16) uint8, error map) of `img` under the preset `prof`; `key` names the content."""
    k = (fmt, key, prof)
    if k not in _cache:
        enc = (oracle.encode_mt if mt else oracle.encode)(fmt, img, prof).reshape(-1, 16)
        enc.setflags(write=False)
        _cache[k] = enc
    km = (fmt, key, prof, mask)
    if km not in _cache:
        e = block_errors(oracle, fmt, _cache[k], img, mask)
        e.setflags(write=False)
        _cache[km] = e
    return _cache[k], _cache[km]


def predict(oracle, fmt, key, img, first, refine, mask, budget, mt=False):
    """dict: target (n, 16), block_sse, tier_map, and the seven fields of itw_refine_stats, by the rule."""
    a, ea = tier(oracle, fmt, key, img, first, mask, mt)
    b, eb = tier(oracle, fmt, key, img, refine, mask, mt)
    listed = ea > budget if budget < U64_MAX else np.zeros(ea.shape, dtype=bool)
    won = listed & (eb < ea)
    final = np.where(won, eb, ea)
    return {"target": np.where(won[:, None], b, a), "block_sse": final, "tier_map": listed.astype(np.uint8) + won.astype(np.uint8),
            "blocks": int(ea.size), "listed": int(listed.sum()), "replaced": int(won.sum()), "sse_first": int(ea.sum()),
            "sse_final": int(final.sum()), "worst_first": int(ea.max()), "worst_final": int(final.max())}


def same(got, want, what=""):
    """got: (blocks, RefineStats, block_sse, tier_map) as compress_refined returns them (numpy or CUDA tensors); every comparison is ==."""
    from conftest import first_mismatch
    host = [x.cpu().numpy() if hasattr(x, "data_ptr") else x for x in (got[0], got[2], got[3])]
    m = first_mismatch(host[0], want["target"], 16)
    assert m is None, (what, m)
    st = got[1].as_dict()
    for f in STATS:
        assert st[f] == want[f], (what, f, st[f], want[f])
    assert np.array_equal(host[1].astype(np.int64), want["block_sse"]), (what, "block_sse")
    assert np.array_equal(host[2], want["tier_map"]), (what, "tier_map")


def to_gpu(gpu, a):
    import torch
    return torch.from_numpy(np.array(a.view(np.int16) if a.dtype == np.uint16 else a)).to(gpu)      # (a copy: the content is frozen)
