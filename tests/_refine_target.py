"""What itwCompressImageRefinedTo has to return, predicted by the CPU oracle alone (tests/test_gpu_refine_target.py and
test_gpu_refine_target_extents.py), on top of tests/_refine.py's tier, predict and same.

select(e, k): np.sort(e)[::-1][k], 0 past the end.  Policy A is _refine.predict with that budget.  Policy B is a plain simulation of the
rounds of include/itw_dispatch.h from the oracle's two encodings and their two error maps.  Nothing here is derived from the library."""
import numpy as np

import _refine as R

U64_MAX = R.U64_MAX
ROUNDS = 5


def select(e, k):
    """The (k+1)-th largest of `e` counting multiplicity, 0 if there are at most k values."""
    return int(np.sort(e)[::-1][k]) if k < e.size else 0


def quota(nb, j):
    return max(1, nb >> (4 - j)) if j < 4 else nb


def predict(oracle, fmt, key, img, first, refine, mask, max_listed=U64_MAX, target=U64_MAX, mt=False):
    """dict: _refine.predict's fields over the whole call, plus rounds, target_met, budget[5], listed_per_round[5]."""
    a, ea = R.tier(oracle, fmt, key, img, first, mask, mt)
    b, eb = R.tier(oracle, fmt, key, img, refine, mask, mt)
    nb = int(ea.size)
    if target == U64_MAX:                                        # policy A: one round over all blocks
        t = select(ea, max_listed)
        want = dict(R.predict(oracle, fmt, key, img, first, refine, mask, t, mt))
        want.update(rounds=1, target_met=1, budget=[t, 0, 0, 0, 0], listed_per_round=[want["listed"], 0, 0, 0, 0])
        return want
    tmap = np.zeros(nb, dtype=np.uint8)
    cur = ea.copy()
    took = np.zeros(nb, dtype=bool)
    budget, per_round, rounds, cap_left = [0] * ROUNDS, [0] * ROUNDS, 0, max_listed
    for j in range(ROUNDS):
        if int(cur.sum()) <= target or cap_left == 0:
            break
        rounds += 1
        cand = tmap == 0
        t = select(cur[cand], min(cap_left, quota(nb, j)))
        listed = cand & (cur > t)
        won = listed & (eb < ea)
        tmap[listed] = 1
        tmap[won] = 2
        took |= won
        cur = np.where(won, eb, cur)
        budget[j], per_round[j] = t, int(listed.sum())
        cap_left -= per_round[j]
    return {"target": np.where(took[:, None], b, a), "block_sse": cur, "tier_map": tmap, "blocks": nb, "listed": int((tmap > 0).sum()),
            "replaced": int(took.sum()), "sse_first": int(ea.sum()), "sse_final": int(cur.sum()), "worst_first": int(ea.max()),
            "worst_final": int(cur.max()), "rounds": rounds, "target_met": int(int(cur.sum()) <= target), "budget": budget,
            "listed_per_round": per_round}


class _Total:
    """RefineTargetStats seen as _refine.same wants its stats."""

    def __init__(self, st):
        self.st = st

    def as_dict(self):
        return self.st.total.as_dict()


def same(got, want, what=""):
    """got: (blocks, RefineTargetStats, block_sse, tier_map) as compress_refined_to returns them; every comparison is ==."""
    st = got[1]
    R.same((got[0], _Total(st), got[2], got[3]), want, what)
    assert int(st.rounds) == want["rounds"], (what, "rounds", int(st.rounds), want["rounds"])
    assert int(st.target_met) == want["target_met"], (what, "target_met", int(st.target_met), want["target_met"])
    assert [int(v) for v in st.budget] == want["budget"], (what, "budget", list(st.budget), want["budget"])
    assert [int(v) for v in st.listed] == want["listed_per_round"], (what, "listed", list(st.listed), want["listed_per_round"])
