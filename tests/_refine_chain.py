"""What itwCompressImageChainRefined[To] has to return, predicted by the CPU oracle alone (tests/test_gpu_refine_chain.py and
test_gpu_refine_chain_extents.py), on top of tests/_refine.py and tests/_refine_target.py.

Per image: np.pad(mode="edge") to multiples of 4, oracle.encode under a preset, oracle.decode at the padded size, the squared differences
of the channels in the mask with the rows >= h and the columns >= w zeroed -- padding is not compared -- reduced per block.  The blocks and
the maps of the images are concatenated, and the chain is then ONE population: _refine.predict's rule and _refine_target.predict's rounds
run over the concatenated maps.  They take their two encodings and error maps from _refine.tier, whose store this module fills for a
chain's key; nothing here is derived from the library.  Per-image stats are the same seven fields over slices of the same arrays."""
import numpy as np

import _refine as R
import _refine_target as T

U64_MAX = R.U64_MAX

_uncropped = {}


def starts(images):
    """First block of every image in the chain's concatenated block list, and the total."""
    n = [((im.shape[1] + 3) // 4) * ((im.shape[0] + 3) // 4) for im in images]
    return [int(v) for v in np.cumsum([0] + n[:-1])], int(sum(n))


def _image(oracle, fmt, img, prof):
    """(blocks (n, 16), squared differences (ph, pw, 4) int64 over the PADDED image) of one image under `prof`."""
    h, w = img.shape[:2]
    padded = np.ascontiguousarray(np.pad(img, ((0, -h % 4), (0, -w % 4), (0, 0)), mode="edge"))
    enc = oracle.encode(fmt, padded, prof).reshape(-1, 16)
    dec, _ = oracle.decode(fmt, enc, padded.shape[1], padded.shape[0])
    if fmt == "bc6h":                                            # the decoders fill alpha with 1.0
        full = np.empty(padded.shape, dtype=np.uint16)
        full[..., :3] = dec
        full[..., 3] = 0x3C00
        dec = full
    d = padded.astype(np.int64) - dec.astype(np.int64)
    return enc, d * d


def _per_block(sq, mask):
    ph, pw = sq.shape[:2]
    return sq[..., [c for c in range(4) if mask >> c & 1]].sum(axis=2).reshape(ph // 4, 4, pw // 4, 4).sum(axis=(1, 3)).reshape(-1)


def tier(oracle, fmt, key, images, prof, mask):
    """(blocks (n, 16), error map, error map WITH the padding counted) of the chain `images` under `prof`; `key` names the content.
    Computed once and frozen; the first two are also what _refine.tier returns for (fmt, key, prof, mask) from here on."""
    k, km = (fmt, key, prof), (fmt, key, prof, mask)
    if km not in _uncropped:
        if (k, "sq") not in _uncropped:
            per = [_image(oracle, fmt, im, prof) for im in images]
            enc = np.concatenate([p[0] for p in per])
            enc.setflags(write=False)
            R._cache[k] = enc
            _uncropped[(k, "sq")] = [p[1] for p in per]
        crop, full = [], []
        for im, sq in zip(images, _uncropped[(k, "sq")]):
            h, w = im.shape[:2]
            full.append(_per_block(sq, mask))
            inside = sq.copy()
            inside[h:] = 0
            inside[:, w:] = 0
            crop.append(_per_block(inside, mask))
        e, u = np.concatenate(crop), np.concatenate(full)
        e.setflags(write=False)
        u.setflags(write=False)
        R._cache[km] = e
        _uncropped[km] = u
    return R._cache[k], R._cache[km], _uncropped[km]


def image_stats(want, ea, images):
    """The seven fields over every image's slice of the maps of a prediction; `ea` is the first tier's map."""
    first, total = starts(images)
    out = []
    for a, b in zip(first, first[1:] + [total]):
        t, fin, e = want["tier_map"][a:b], want["block_sse"][a:b], ea[a:b]
        out.append({"blocks": b - a, "listed": int((t > 0).sum()), "replaced": int((t == 2).sum()), "sse_first": int(e.sum()),
                    "sse_final": int(fin.sum()), "worst_first": int(e.max()), "worst_final": int(fin.max())})
    return out


def predict(oracle, fmt, key, images, first, refine, mask, budget):
    """_refine.predict's dict over the chain, plus image_stats."""
    ea = tier(oracle, fmt, key, images, first, mask)[1]
    tier(oracle, fmt, key, images, refine, mask)
    want = dict(R.predict(oracle, fmt, key, None, first, refine, mask, budget))
    want["image_stats"] = image_stats(want, ea, images)
    return want


def predict_to(oracle, fmt, key, images, first, refine, mask, max_listed=U64_MAX, target=U64_MAX):
    """_refine_target.predict's dict over the chain, plus image_stats."""
    ea = tier(oracle, fmt, key, images, first, mask)[1]
    tier(oracle, fmt, key, images, refine, mask)
    want = dict(T.predict(oracle, fmt, key, None, first, refine, mask, max_listed, target))
    want["image_stats"] = image_stats(want, ea, images)
    return want


def same_images(per, want, what=""):
    assert len(per) == len(want["image_stats"]), (what, len(per))
    for i, (got, exp) in enumerate(zip(per, want["image_stats"])):
        st = got.as_dict()
        for f in R.STATS:
            assert st[f] == exp[f], (what, "image", i, f, st[f], exp[f])
    for f in ("blocks", "listed", "replaced", "sse_first", "sse_final"):
        assert sum(int(getattr(p, f)) for p in per) == want[f], (what, "sum of", f)
    for f in ("worst_first", "worst_final"):
        assert max(int(getattr(p, f)) for p in per) == want[f], (what, "max of", f)


def same(got, want, what=""):
    """got: (blocks, RefineStats, block_sse, tier_map, image_stats) as compress_chain_refined returns them; every comparison is ==."""
    R.same(got[:4], want, what)
    same_images(got[4], want, what)


def same_to(got, want, what=""):
    """got: (blocks, RefineTargetStats, block_sse, tier_map, image_stats) as compress_chain_refined_to returns them."""
    T.same(got[:4], want, what)
    same_images(got[4], want, what)
