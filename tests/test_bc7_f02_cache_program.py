"""csrc/bc7_f02_schedule.h (tools/gen_bc7_f02_schedule.py): the visiting order of the three-subset shapes and the two cache programs that
search_02 (csrc/bc7.hip) runs over it -- BC7_F02_SCHEDULE, mode 2's subset errors in four slots, and BC7_F02_SCHEDULE_EXT, mode 0's in four more.
Both are re-simulated here from the arrays and the mask table alone, the way the kernel reads them, and held against what the header's
comment states.  No GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "intel-texture-works-plugin_amd", "csrc")


def _array(text, name, n):
    body = text[text.index(name):]
    body = body[body.index("{") + 1:body.index("}")]
    v = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]+)u", body)]
    assert len(v) == n, (name, len(v))
    return v


def _load():
    with open(os.path.join(CSRC, "bc7_tables.h")) as f:
        masks = _array(f.read(), "BCN_SUBSET_MASKS[128]", 128)
    with open(os.path.join(CSRC, "bc7_f02_schedule.h")) as f:
        header = f.read()
    subsets = []
    for shape in range(64, 128):
        m0, m1 = masks[shape] & 0xffff, masks[shape] >> 16
        subsets.append((m0, m1, ~(m0 | m1) & 0xffff))
    return header, subsets, _array(header, "BC7_F02_SCHEDULE[64]", 64), _array(header, "BC7_F02_SCHEDULE_EXT[64]", 64)


def _acts(prim, ext, pos, j):
    """(mode 2 act, slot), (mode 0 act, slot) of subset j at a position, as search_02 extracts them"""
    return ((prim[pos] >> (8 + 4 * j)) & 3, (prim[pos] >> (10 + 4 * j)) & 3), ((ext[pos] >> (4 * j)) & 3, (ext[pos] >> (4 * j + 2)) & 3)


def _run(subsets, prim, ext):
    """Runs both programs.  Every load must find, in its slot, the mask it stands for, put there by a position that computed that mode and not
    overwritten since.  Returns what the scan still computes."""
    slots2, slots0 = {}, {}
    seen = dict(eval0=[], eval2=[], fits=[], third_stats=0, load0=0, load2=0, skipped=0)
    for pos in range(64):
        part = prim[pos] & 63
        do0 = part < 16
        rest_valid = True
        for j in range(3):
            mask = subsets[part][j]
            (act2, slot2), (act0, slot0) = _acts(prim, ext, pos, j)
            assert act2 in (0, 1, 2) and act0 in (0, 1, 2), (pos, j)
            if not do0:
                assert act0 == 0 and slot0 == 0, ("a mode 0 act at a shape mode 0 does not have", pos, part, j)
            load2, load0 = act2 == 2, act0 == 2
            if load2:
                assert slots2.get(slot2) == mask, ("mode 2", pos, j, hex(mask))
                seen["load2"] += 1
            if load0:
                assert slots0.get(slot0) == mask, ("mode 0", pos, j, hex(mask))
                seen["load0"] += 1
            need0 = do0 and not load0
            if load2 and not need0:
                seen["skipped"] += 1
                rest_valid = False
                continue
            seen["fits"].append(mask)
            if j == 2 and not rest_valid:
                seen["third_stats"] += 1
            if need0:
                seen["eval0"].append(mask)
                if act0 == 1:
                    slots0[slot0] = mask                     # a store happens only where the mode was computed
            else:
                assert act0 != 1, ("a mode 0 store without a computation", pos, j)
            if not load2:
                seen["eval2"].append(mask)
                if act2 == 1:
                    slots2[slot2] = mask
    return seen


def test_every_shape_is_visited_once():
    _, _, prim, ext = _load()
    assert sorted(w & 63 for w in prim) == list(range(64))
    assert all(w < (1 << 20) for w in prim) and all(x < (1 << 12) for x in ext)


def test_both_programs_load_what_was_stored():
    _, subsets, prim, ext = _load()
    seen = _run(subsets, prim, ext)
    # every mask is still evaluated at least once per mode that sees it, and fitted at least once
    assert set(seen["eval2"]) == set(seen["fits"]) == {m for s in subsets for m in s}
    assert set(seen["eval0"]) == {m for s in subsets[:16] for m in s}


def test_the_primary_array_alone_is_a_valid_program():
    """The kernels without room for the mode 0 slots run BC7_F02_SCHEDULE with a zero extension word."""
    _, subsets, prim, _ = _load()
    seen = _run(subsets, prim, [0] * 64)
    assert seen["load0"] == 0 and len(seen["eval0"]) == 48
    assert seen["load2"] >= 46


def test_the_headers_counts_equal_a_re_simulation():
    header, subsets, prim, ext = _load()
    seen = _run(subsets, prim, ext)
    m = re.search(r"loads: mode 0 (\d+), mode 2 (\d+); subsets skipped outright: (\d+) of 192", header)
    assert m, "the header's comment lost its counts"
    assert (seen["load0"], seen["load2"], seen["skipped"]) == tuple(int(g) for g in m.groups())
    m = re.search(r"left repeated: \(mask, mode 0\) evaluations (\d+), \(mask, mode 2\) evaluations (\d+), fits (\d+); "
                  r"third subsets summed by stats_int: (\d+)", header)
    assert m, "the header's comment lost its counts"
    left = (len(seen["eval0"]) - len(set(seen["eval0"])), len(seen["eval2"]) - len(set(seen["eval2"])),
            len(seen["fits"]) - len(set(seen["fits"])), seen["third_stats"])
    assert left == tuple(int(g) for g in m.groups())
    # 36 distinct masks in mode 0's 48 subsets, 140 in mode 2's 192: what is loaded and what is left repeated add up to the repeats there are
    assert seen["load0"] + left[0] == 48 - 36 and seen["load2"] + left[1] == 192 - 140
    assert len(seen["fits"]) + seen["skipped"] == 192


def test_every_combination_wins_on_the_partition_surface():
    """The input condition of tests/test_gpu_bc7_f02_cache.py, on the CPU: on its third content the oracle's stream holds a block of mode 0 with
    each of its 16 partitions and a block of mode 2 with each of its 64, under both profiles, at the smaller of the two sizes that can hold them."""
    import _f02_surfaces as fs
    from oracle import pyoracle
    pyoracle.build()
    img = fs.partitions(96, 128)
    for prof in fs.PROFILES:
        missing = fs.missing_winners(pyoracle.encode_mt("bc7", img, prof))
        assert not missing, (prof, sorted(missing))
