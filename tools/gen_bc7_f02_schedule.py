"""Generates csrc/bc7_f02_schedule.h: the visiting order of the 64 three-subset shapes (BC7 modes 0/2) and two static
cache programs for subset results, one per mode.

Why: 192 (shape, subset) pairs of the three-subset table use only 140 distinct texel masks, and everything the scan
computes for a subset -- moments, line fit, endpoint codes, per-texel indices and errors -- depends on the mask alone.
Modes 0/2 take every shape with a strict `<` in table order, so the winner is "lowest error, then lowest table index"
whatever the visiting order; the scan is therefore free to visit shapes so that equal masks come close together and to
keep the last few subset errors of each mode at hand.  Mode 2 sees all 64 shapes (140 masks in 192 subsets); mode 0 sees
the first 16 (36 masks in 48 subsets), so its program acts only at positions whose shape has table index < 16.

The order is chosen for both programs together; the objective is the estimated VALU instructions a wave still executes
(COST below: a subset's fit, its mode 0 part, its mode 2 part, its moments summed or taken by subtraction).  A subset
with every result it needs loaded is skipped outright; one that loads a single mode keeps its fit.  The third subset's
moments come by subtraction from the block's unless one of the first two was skipped outright (evaluating the skipped
subset last instead would save nothing: the subtraction needs both other subsets' moments, and the two subsets that are
left to compute are summed whichever of them comes last).

Primary word per position (BC7_F02_SCHEDULE, a valid four-slot mode 2 program on its own; the kernels without room for
more run it alone):  shape | act0 << 8 | slot0 << 10 | act1 << 12 | slot1 << 14 | act2 << 16 | slot2 << 18
Extension word per position (BC7_F02_SCHEDULE_EXT), the mode 0 program:  act0 << 4j | slot0 << (4j+2) for subset j
  act: 0 compute, 1 compute and store into slot, 2 load from slot.
K2 mode 2 slots, K0 mode 0 slots, Belady (farthest next use) eviction in each.  The scan kernel has room for four more
32-bit slots per lane and all of them go to mode 0, which then catches 11 of its 12 repeats; more mode 2 slots could
catch at most the 2 mode 2 repeats that four leave.
Run: python tools/gen_bc7_f02_schedule.py  (reads csrc/bc7_tables.h)."""
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "intel-texture-works-plugin_amd", "csrc")
K2 = 4           # mode 2 slots (primary word)
K0 = 4           # mode 0 slots (extension word)
# estimated VALU instructions per wave of: a line fit, the mode 0 part, the mode 2 part, moments by stats_int, by subtraction
COST = {"fit": 300, "m0": 150, "m2": 100, "stats": 48, "sub": 9}


def subsets():
    t = open(os.path.join(CSRC, "bc7_tables.h")).read()
    body = t[t.index("BCN_SUBSET_MASKS[128]"):]
    body = body[body.index("{"):body.index("}")]
    masks = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]+)u", body)]
    out = []
    for i in range(64, 128):
        m0, m1 = masks[i] & 0xffff, masks[i] >> 16
        out.append([m0, m1, ~(m0 | m1) & 0xffff])
    return out


def belady(order, S3, k, member):
    """One cache program over the positions whose shape satisfies `member`: acts[pos][j] = (act, slot).  Low slots first."""
    uses = {}
    for pos, s in enumerate(order):
        if member(s):
            for m in S3[s]:
                uses.setdefault(m, []).append(pos)
    cache, free = {}, list(range(k))
    acts = []
    for pos, s in enumerate(order):
        row = [(0, 0)] * 3
        if member(s):
            for j, m in enumerate(S3[s]):
                nxt = [p for p in uses[m] if p > pos]
                act, slot = 0, 0
                if m in cache:
                    act, slot = 2, cache[m]
                    if not nxt:
                        free.append(cache.pop(m))
                elif nxt and k:
                    if not free:
                        def next_use(mm):
                            f = [p for p in uses[mm] if p > pos]
                            return f[0] if f else 10 ** 9
                        victim = max(cache, key=next_use)
                        if next_use(victim) > nxt[0]:
                            free.append(cache.pop(victim))
                    if free:
                        free.sort()
                        slot = free.pop(0)
                        cache[m] = slot
                        act = 1
                row[j] = (act, slot)
        acts.append(row)
    return acts


def account(order, a2, a0):
    """What the scan still does under the two programs: estimated instructions and the counts the header states."""
    c = dict(cost=0, eval0=0, eval2=0, fits=0, third_stats=0, load0=0, load2=0, skipped=0)
    for pos, s in enumerate(order):
        rest_valid = True
        for j in range(3):
            need0 = s < 16 and a0[pos][j][0] != 2
            need2 = a2[pos][j][0] != 2
            c["load0"] += s < 16 and not need0
            c["load2"] += not need2
            if not need0 and not need2:
                c["skipped"] += 1
                rest_valid = False
                continue
            c["fits"] += 1
            c["eval0"] += need0
            c["eval2"] += need2
            summed = j < 2 or not rest_valid
            c["third_stats"] += j == 2 and summed
            c["cost"] += COST["fit"] + (COST["stats"] if summed else COST["sub"]) + COST["m0"] * need0 + COST["m2"] * need2
    return c


def simulate(order, S3):
    a2 = belady(order, S3, K2, lambda s: True)
    a0 = belady(order, S3, K0, lambda s: s < 16)
    return account(order, a2, a0), a2, a0


def words_of(order, a2, a0):
    prim, ext = [], []
    for pos, s in enumerate(order):
        w, x = s, 0
        for j in range(3):
            act2, slot2 = a2[pos][j]
            act0, slot0 = a0[pos][j]
            w |= (act2 << (8 + 4 * j)) | (slot2 << (10 + 4 * j))
            x |= (act0 << (4 * j)) | (slot0 << (4 * j + 2))
        prim.append(w); ext.append(x)
    return prim, ext


def main():
    S3 = subsets()
    masks0 = set(m for s in range(16) for m in S3[s])
    masks2 = set(m for s in range(64) for m in S3[s])
    random.seed(7)
    best = None
    for trial in range(1500):
        rem = set(range(64))
        cur = random.choice(list(rem))
        order = [cur]; rem.remove(cur)
        while rem:
            recent = set(m for o in order[-4:] for m in S3[o])
            nxt = max(rem, key=lambda r: (len(set(S3[r]) & recent), random.random()))
            order.append(nxt); rem.remove(nxt)
        c = simulate(order, S3)[0]["cost"]
        if best is None or c < best[0]:
            best = (c, order)
    cost, order = best
    improved = True
    while improved:                                   # local improvement: pairwise swaps, then moving one shape
        improved = False
        for a in range(64):
            for b in range(64):
                if a == b:
                    continue
                o2 = order[:]; o2[a], o2[b] = o2[b], o2[a]
                o3 = order[:]; o3.insert(b, o3.pop(a))
                for o in (o2, o3):
                    c = simulate(o, S3)[0]["cost"]
                    if c < cost:
                        cost, order, improved = c, o, True
    assert sorted(order) == list(range(64))
    c, a2, a0 = simulate(order, S3)
    prim, ext = words_of(order, a2, a0)
    table = account(list(range(64)), [[(0, 0)] * 3] * 64, [[(0, 0)] * 3] * 64)
    rep0, rep2, repf = c["eval0"] - len(masks0), c["eval2"] - len(masks2), c["fits"] - len(masks2)
    assert sum(((w >> (8 + 4 * j)) & 3) == 2 for w in prim for j in range(3)) >= 46
    out = ["/* GENERATED by tools/gen_bc7_f02_schedule.py -- do not edit.",
           " * Visiting order of the three-subset shapes and the static cache schedules of subset results: mode 2 in %d slots, mode 0 in %d."
           % (K2, K0),
           " * BC7_F02_SCHEDULE: shape | act_j << (8+4j) | slot_j << (10+4j), the mode 2 program (valid on its own).",
           " * BC7_F02_SCHEDULE_EXT: act0_j << 4j | slot0_j << (4j+2), the mode 0 program (shapes with table index < 16 only).",
           " * act: 0 compute, 1 compute + store, 2 load.",
           " * loads: mode 0 %d, mode 2 %d; subsets skipped outright: %d of 192."
           % (c["load0"], c["load2"], c["skipped"]),
           " * left repeated: (mask, mode 0) evaluations %d, (mask, mode 2) evaluations %d, fits %d; third subsets summed by stats_int: %d."
           % (rep0, rep2, repf, c["third_stats"]),
           " * estimated VALU instructions per wave (COST of the generator): %d, against %d in table order with nothing cached. */"
           % (c["cost"], table["cost"]),
           "BCN_TABLE_QUAL unsigned int BC7_F02_SCHEDULE[64] = {"]
    for i in range(0, 64, 8):
        out.append("    " + " ".join("0x%05xu," % w for w in prim[i:i + 8]))
    out.append("};")
    out.append("BCN_TABLE_QUAL unsigned int BC7_F02_SCHEDULE_EXT[64] = {")
    for i in range(0, 64, 8):
        out.append("    " + " ".join("0x%03xu," % w for w in ext[i:i + 8]))
    out.append("};")
    open(os.path.join(CSRC, "bc7_f02_schedule.h"), "w").write("\n".join(out) + "\n")
    print("\n".join(out[1:8]))
    print("order", order)


if __name__ == "__main__":
    main()
