"""Every launch switch the library reads once per process (csrc/bc7.hip env_once: ITW_BC7_FUSED, _BOUND, _ALPHA_PRUNE, _BANDS, _COMPACT,
ITW_STAGED_BANDS, ITW_BC7_PATH as a variable; csrc/abi.hip: ITW_STAGED_VERDICT_THR, ITW_STAGED_WIDE_MAX), each in a fresh child process
(tests/_launch_switch_child.py) at the smallest shapes that still switch.  Two assertions per row:
  bytes   every stream the child produced equals the oracle's, block for block;
  route   every call's route witness (include/itw_test_hooks.h itwTestBc7RouteCounters, the hooks build only) equals the tables below --
          written down from the rules above Bc7Modes, bc7_use_wide, launch_bc7, two_bands, launch_rgb_bounded (csrc/bc7.hip) and launch(),
          compress_runs (csrc/abi.hip), never by asking the library.  A switch test without it passes as well when a variable is renamed or
          a threshold moves above the test's size.
At most one child is alive at a time; a child that ends abnormally fails its row and every later row is not started.

Where the tables differ from what one would first write down:
  * ITW_BC7_PATH=deep makes bc7_wide_block_limit -1, so under it a STAGED run of a host-pointer call takes the fused shape, never the wide
    one: in the deep rows ITW_STAGED_WIDE_MAX shows nothing and ITW_STAGED_VERDICT_THR=0 shows in the launch shapes only.  Two further rows
    without ITW_BC7_PATH run the same battery by size (every call here is small: the device-resident part goes wide) and there the staged
    runs are WIDE, or -- ITW_STAGED_WIDE_MAX=1 -- RGB_BOUNDED.
  * A PROBE is a launch_bc7 call of its own: it counts RGB_BOUNDED (and PAIRS, ROT_TASKS, COMPACT: its band is built like any other) besides
    HOST_VERDICT and PROBE.
  * The first run of the host-pointer calls is longer than in tests/test_gpu_host_runs_small.py: see HOST_RUNS in the child.
  * Whether a later run of a call sees the call's own estimate is a race (compress_runs polls an event): where the estimate changes the shape,
    every split of the remaining runs is listed and nothing else.  Where ITW_STAGED_VERDICT_THR is unset the estimate's value depends on
    the content (80 %): both shapes are listed for `slow`; the rows that set it to 0 and 100 pin each.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import _launch_switch_child as child
from conftest import first_mismatch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# One child, measured on an MI355X (the defaults row, which also runs the product library): 2.4 s wall, nearly all of it importing torch and
# loading the code objects.  Ten times that, rounded up to a multiple of 30 s.
LIMIT = 30

DEEP = {"ITW_BC7_PATH": "deep"}
#        row id              environment                                                          device table   host table
ROWS = [("defaults",         {**DEEP},                                                            "default",     "deep"),
        ("fused0",           {**DEEP, "ITW_BC7_FUSED": "0"},                                      "per_family",  "per_family"),
        ("bound0",           {**DEEP, "ITW_BC7_BOUND": "0"},                                      "bound0",      "bound0"),
        ("alpha_prune0",     {**DEEP, "ITW_BC7_ALPHA_PRUNE": "0"},                                "alpha_prune0", "alpha_prune0"),
        ("bands1",           {**DEEP, "ITW_BC7_BANDS": "1"},                                      "bands1",      "deep"),
        ("compact0",         {**DEEP, "ITW_BC7_COMPACT": "0"},                                    "compact0",    "compact0"),
        ("compact0_bands1",  {**DEEP, "ITW_BC7_COMPACT": "0", "ITW_BC7_BANDS": "1"},              "compact0_bands1", "compact0"),
        ("staged_bands0",    {**DEEP, "ITW_STAGED_BANDS": "0"},                                   "default",     "staged_bands0"),
        ("verdict_thr100",   {**DEEP, "ITW_STAGED_VERDICT_THR": "100"},                           "default",     "deep_thr100"),
        ("verdict_thr0",     {**DEEP, "ITW_STAGED_VERDICT_THR": "0"},                             "default",     "deep_thr0"),
        ("verdict_thr0_wide_max1", {**DEEP, "ITW_STAGED_VERDICT_THR": "0", "ITW_STAGED_WIDE_MAX": "1"}, "default", "deep_thr0"),
        ("fused0_verdict_thr0", {**DEEP, "ITW_BC7_FUSED": "0", "ITW_STAGED_VERDICT_THR": "0"},    "per_family",  "per_family"),
        ("path_wide",        {"ITW_BC7_PATH": "wide"},                                            "wide",        "path_wide"),
        # by size (no ITW_BC7_PATH): where the staged runs can go wide
        ("by_size_verdict_thr0", {"ITW_STAGED_VERDICT_THR": "0"},                                 "wide",        "by_size_thr0"),
        ("by_size_verdict_thr0_wide_max1", {"ITW_STAGED_VERDICT_THR": "0", "ITW_STAGED_WIDE_MAX": "1"}, "wide",  "by_size_thr0_wide_max1")]
ROW_VARIABLES = sorted({k for _, env, _, _ in ROWS for k in env})

# ---- the device-resident part: one launch() of shape WHOLE, one launch_bc7 ---------------------------------------------------------------
# Bc7Modes of the five structs: `slow` rgb_bounded; `alpha_slow` alpha_first + bounded + mode 7 unranked -> ALPHA_FIRST_BOUNDED7; with mode 7
# ranked (3) -> launch_alpha_first with M.bounded; `basic` ranked lists, nothing bounded -> the reference's order; `alpha_basic` alpha_first, not
# bounded.  two_bands: 33 chunks (A) >= 32, 3 chunks (B) not; the pilot goes with two bands whatever its threshold (0 and 100 are both >= 0).
# "A/slow" is the `unset` knob; the other three per-call knobs follow from it (KNOB_DROPS).
SLOW_2 = "SHAPE_WHOLE RGB_BOUNDED TWO_BANDS PILOT PAIRS ROT_TASKS COMPACT"
SLOW_1 = "SHAPE_WHOLE RGB_BOUNDED PAIRS ROT_TASKS COMPACT"
DEFAULT = {"A/slow": SLOW_2, "A_unaligned/slow": SLOW_2, "B/slow": SLOW_1,
           "A/alpha_slow": "SHAPE_WHOLE ALPHA_FIRST_BOUNDED7 TWO_BANDS", "B/alpha_slow": "SHAPE_WHOLE ALPHA_FIRST_BOUNDED7",
           "A/basic": "SHAPE_WHOLE REFERENCE_ORDER", "B/basic": "SHAPE_WHOLE REFERENCE_ORDER",
           "A/alpha_basic": "SHAPE_WHOLE ALPHA_FIRST_PLAIN", "B/alpha_basic": "SHAPE_WHOLE ALPHA_FIRST_PLAIN",
           "A/alpha_slow_ranked7": "SHAPE_WHOLE ALPHA_FIRST_BOUNDED", "B/alpha_slow_ranked7": "SHAPE_WHOLE ALPHA_FIRST_BOUNDED"}
REF = "SHAPE_WHOLE REFERENCE_ORDER"
DEVICE = {
    "default": DEFAULT,
    "per_family": {k: "SHAPE_WHOLE PER_FAMILY" for k in DEFAULT},
    "wide": {k: "SHAPE_WHOLE WIDE" for k in DEFAULT},              # all five structs are within what bc7_use_wide supports
    # ITW_BC7_BOUND=0: nothing is bounded -- `slow` in the reference's order, both alpha_slow structs alpha-first without a bound
    "bound0": {**DEFAULT, "A/slow": REF, "A_unaligned/slow": REF, "B/slow": REF,
               "A/alpha_slow": "SHAPE_WHOLE ALPHA_FIRST_PLAIN", "B/alpha_slow": "SHAPE_WHOLE ALPHA_FIRST_PLAIN",
               "A/alpha_slow_ranked7": "SHAPE_WHOLE ALPHA_FIRST_PLAIN", "B/alpha_slow_ranked7": "SHAPE_WHOLE ALPHA_FIRST_PLAIN"},
    # ITW_BC7_ALPHA_PRUNE=0: no alpha_first; an RGBA struct has mode 7 on, so it is not rgb_bounded either
    "alpha_prune0": {**DEFAULT, "A/alpha_slow": REF, "B/alpha_slow": REF, "A/alpha_basic": REF, "B/alpha_basic": REF,
                     "A/alpha_slow_ranked7": REF, "B/alpha_slow_ranked7": REF},
    "bands1": {**DEFAULT, "A/slow": SLOW_1, "A_unaligned/slow": SLOW_1, "A/alpha_slow": "SHAPE_WHOLE ALPHA_FIRST_BOUNDED7"},
    "compact0": {**DEFAULT, "A/slow": "SHAPE_WHOLE RGB_BOUNDED TWO_BANDS PILOT PAIRS ROT_TASKS", "A_unaligned/slow": "SHAPE_WHOLE RGB_BOUNDED TWO_BANDS PILOT PAIRS ROT_TASKS",
                 "B/slow": "SHAPE_WHOLE RGB_BOUNDED PAIRS ROT_TASKS"},
    "compact0_bands1": {**DEFAULT, "A/slow": "SHAPE_WHOLE RGB_BOUNDED PAIRS ROT_TASKS", "A_unaligned/slow": "SHAPE_WHOLE RGB_BOUNDED PAIRS ROT_TASKS",
                        "B/slow": "SHAPE_WHOLE RGB_BOUNDED PAIRS ROT_TASKS", "A/alpha_slow": "SHAPE_WHOLE ALPHA_FIRST_BOUNDED7"},
}
# what a per-call knob takes out of a launch_rgb_bounded call (ITW_BC7_PAIR_CAP=1 only overflows the buckets: the pair route stays on)
KNOB_DROPS = {"unset": (), "pairs0": ("PAIRS",), "paircap1": (), "rot0": ("ROT_TASKS",)}

# ---- the host-pointer part: three runs per call (compress_runs), each a launch() of some shape and a launch_bc7 -------------------------------
# What ONE launch of a shape counts in bc7.hip, per profile ("*": every shape not named).  Every run is below 32 chunks: one band.  A band is
# `single`: never wide.  STAGED / WHOLE runs: wide where bc7_use_wide allows it -- never under ITW_BC7_PATH=deep.
SLOW_RUN = "RGB_BOUNDED PAIRS ROT_TASKS COMPACT"
SLOW_DEEP = {"*": SLOW_RUN, "VERDICT_BAND": SLOW_RUN + " HOST_VERDICT", "PROBE": SLOW_RUN + " HOST_VERDICT PROBE"}
SLOW_NOCOMPACT = {k: v.replace(" COMPACT", "") for k, v in SLOW_DEEP.items()}
HOST_ROUTES = {
    "deep":          {"slow": SLOW_DEEP, "alpha_slow": {"*": "ALPHA_FIRST_BOUNDED7"}, "basic": {"*": "REFERENCE_ORDER"}},
    "compact0":      {"slow": SLOW_NOCOMPACT, "alpha_slow": {"*": "ALPHA_FIRST_BOUNDED7"}, "basic": {"*": "REFERENCE_ORDER"}},
    "per_family":    {"slow": {"*": "PER_FAMILY"}, "alpha_slow": {"*": "PER_FAMILY"}, "basic": {"*": "PER_FAMILY"}},
    "bound0":        {"slow": {"*": "REFERENCE_ORDER"}, "alpha_slow": {"*": "ALPHA_FIRST_PLAIN"}, "basic": {"*": "REFERENCE_ORDER"}},
    "alpha_prune0":  {"slow": SLOW_DEEP, "alpha_slow": {"*": "REFERENCE_ORDER"}, "basic": {"*": "REFERENCE_ORDER"}},
    "path_wide":     {"slow": {"*": "WIDE"}, "alpha_slow": {"*": "WIDE"}, "basic": {"*": "WIDE"}},
    # by size: a STAGED run goes wide up to ITW_STAGED_WIDE_MAX blocks (default 2^20), a WHOLE one up to 262 144
    "by_size":       {"slow": {**SLOW_DEEP, "STAGED": "WIDE", "WHOLE": "WIDE"}, "alpha_slow": {"*": "ALPHA_FIRST_BOUNDED7"}, "basic": {"*": "REFERENCE_ORDER"}},
    "by_size_wide_max1": {"slow": {**SLOW_DEEP, "WHOLE": "WIDE"}, "alpha_slow": {"*": "ALPHA_FIRST_BOUNDED7"}, "basic": {"*": "REFERENCE_ORDER"}},
}
# The shapes of a call's launches, in order, every allowed sequence; "+" joins the two launches of a first run that went wide (the run and its
# probe).  A profile without an order verdict runs as bands wherever bands are allowed.
BANDS = ["VERDICT_BAND BAND BAND"]
FIRST_ESTIMATE_SAYS_WIDE = ["VERDICT_BAND BAND BAND", "VERDICT_BAND BAND STAGED", "VERDICT_BAND STAGED STAGED"]     # read at run 3 / never in time, at run 3, at run 2
WIDE_RUNS = ["STAGED+PROBE STAGED STAGED"]
UNPINNED = FIRST_ESTIMATE_SAYS_WIDE + WIDE_RUNS + ["STAGED+PROBE STAGED BAND", "STAGED+PROBE BAND BAND"]            # ITW_STAGED_VERDICT_THR unset: by content


def _no_verdict(shapes):
    return {"slow": [shapes] * 4, "alpha_slow": [shapes] * 4, "basic": [shapes] * 4, "device_dst": [s.replace("STAGED", "WHOLE") for s in shapes]}


# The last estimate lives in the context a call runs in (abi.hip ThreadCtx::staged_wide, false at first).  The host-to-host calls are offered to
# the combiner and run in ITS context (coalesce_small_call lends it), one after the other; the call into device memory is not combinable and
# runs in the calling thread's own, where it is the first: the shapes of a first call, WHOLE where that has STAGED.
def _verdict(slow_calls, device_dst):
    return {"slow": slow_calls, "alpha_slow": [BANDS] * 4, "basic": [BANDS] * 4, "device_dst": [s.replace("STAGED", "WHOLE") for s in device_dst]}


THR0 = _verdict([FIRST_ESTIMATE_SAYS_WIDE] + [WIDE_RUNS] * 3, FIRST_ESTIMATE_SAYS_WIDE)       # every block row of the photograph lists something: > 0 %
BY_CONTENT = _verdict([FIRST_ESTIMATE_SAYS_WIDE] + [UNPINNED] * 3, FIRST_ESTIMATE_SAYS_WIDE)
#                 host table             routes                 shapes per profile and call
HOST = {"deep":          ("deep",         BY_CONTENT),
        "compact0":      ("compact0",     BY_CONTENT),
        "alpha_prune0":  ("alpha_prune0", BY_CONTENT),
        "per_family":    ("per_family",   _no_verdict(BANDS)),                 # has_order_verdict is false: every call alike, no HOST_VERDICT, no PROBE_IGNORED
        "bound0":        ("bound0",       _no_verdict(BANDS)),
        "staged_bands0": ("deep",         _no_verdict(["STAGED STAGED STAGED"])),
        "path_wide":     ("path_wide",    _no_verdict(["STAGED STAGED STAGED"])),   # bc7_staged_bands_ok: no bands where the wide shape is forced
        "deep_thr100":   ("deep",         _verdict([BANDS] * 4, BANDS)),       # no estimate is above 100 %
        "deep_thr0":     ("deep",         THR0),
        "by_size_thr0":  ("by_size",      THR0),
        "by_size_thr0_wide_max1": ("by_size_wide_max1", THR0)}


def _vector(words):
    """ "NAME NAME=3 ..." -> the counter vector"""
    import itw_amd
    v = np.zeros(len(itw_amd.BC7_ROUTE_COUNTERS), np.int64)
    for word in words.split():
        name, _, count = word.partition("=")
        v[itw_amd.BC7_ROUTE_COUNTERS.index(name)] += int(count or 1)
    return v


def _device_expected(table, case):
    parts = case.split("/")
    if len(parts) == 4:                                               # A/slow/pilot<p>/<knob>
        words = [w for w in DEVICE[table]["A/slow"].split() if w not in KNOB_DROPS[parts[3]]]
        return _vector(" ".join(words))
    return _vector(DEVICE[table][case])


def _host_expected(table, settings, shapes):
    """the vectors of every allowed sequence of launch shapes"""
    routes = HOST_ROUTES[HOST[table][0]][settings]
    out = []
    for seq in shapes:
        v = _vector("")
        for shape in seq.replace("+", " ").split():
            v += _vector("SHAPE_" + shape + " " + routes.get(shape, routes["*"]))
        out.append(v)
    return out


def _named(v):
    import itw_amd
    return {n: int(c) for n, c in zip(itw_amd.BC7_ROUTE_COUNTERS, v) if c}


@pytest.fixture(scope="module")
def battery(oracle, golden_inputs, tmp_path_factory):
    """the child's inputs, saved once, and the oracle's stream of every (image, settings): computed once on the CPU, read-only"""
    from itw_amd import surfaces
    bab = golden_inputs["baboon"]
    images = {}
    for name, (w, h) in child.SHAPES.items():
        half = (w // 8) * 4
        img = surfaces.ldr_smooth(h, w).copy()                        # translucent as generated
        img[:, half:] = surfaces.tile_to(bab, h, w)[:, half:]
        img[:, half:, 3] = 255
        images[name + "_rgba"] = np.ascontiguousarray(img)
        img = img.copy()
        img[..., 3] = 255
        images[name + "_rgb"] = np.ascontiguousarray(img)
    w, h = child.HOST_SHAPE
    images["host_photo"] = np.ascontiguousarray(np.tile(bab[:128, :w], (h // 128, 1, 1)))
    assert images["A_rgb"].shape == (260, 516, 4) and images["host_photo"].shape == (256, 64, 4)

    def settings_of(name):
        s = oracle.bc7_profile(child.profile_of(name))
        if name == "alpha_slow_ranked7":
            s.fastSkipTreshold_mode7 = 3
        return s

    want = {}
    for _, key, st, _, _ in child.device_cases():
        if (key, st) not in want:
            want[key, st] = oracle.encode_mt("bc7", images[key], settings_of(st)).reshape(-1)
    for st in child.HOST_PROFILES:
        want["host_photo", st] = oracle.encode_mt("bc7", images["host_photo"], settings_of(st)).reshape(-1)
    for v in want.values():
        v.setflags(write=False)
    path = str(tmp_path_factory.mktemp("launch_switches") / "inputs.npz")
    np.savez(path, **images)
    return path, want


_abnormal = []          # set by the first child that ends on a signal, aborts or runs into LIMIT: no later row starts anything


def _run_child(inputs, outputs, env_row, product):
    if _abnormal:
        pytest.fail("not started: an earlier child ended abnormally (" + _abnormal[0] + ")")
    env = {k: v for k, v in os.environ.items() if not k.startswith("ITW_")}
    env.update(env_row)
    env["PYTHONPATH"] = os.pathsep.join(p for p in sys.path if p)
    cmd = [sys.executable, os.path.join(ROOT, "tests", "_launch_switch_child.py"), inputs, outputs] + (["--product"] if product else [])
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, timeout=LIMIT)
    except subprocess.TimeoutExpired as e:
        _abnormal.append(f"{env_row}: no end within {LIMIT} s")
        pytest.fail(f"{env_row}: the child did not end within {LIMIT} s\n" + (e.stderr or b"")[-2000:].decode(errors="replace"))
    if r.returncode < 0 or r.returncode in (134, 139):
        _abnormal.append(f"{env_row}: exit status {r.returncode}")
        pytest.fail(f"{env_row}: the child ended abnormally, exit status {r.returncode}\n" + r.stderr[-2000:].decode(errors="replace"))
    assert r.returncode == 0, (env_row, r.returncode, r.stderr[-2000:].decode(errors="replace"))
    return dict(np.load(outputs))


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_switch_row(row, battery, tmp_path):
    name, env_row, device_table, host_table = row
    inputs, want = battery
    got = _run_child(inputs, str(tmp_path / "outputs.npz"), env_row, product=(name == "defaults"))

    # bytes: every stream against the oracle's
    streams = [(case, key, st) for case, key, st, _, _ in child.device_cases()] + [(case, "host_photo", st) for case, st, _ in child.host_cases()]
    for case, key, st in streams:
        bad = first_mismatch(got[case + ".bytes"], want[key, st], 16) if got[case + ".bytes"].size == want[key, st].size else "size differs"
        assert bad is None, (name, key, st, case, bad)
        if name == "defaults" and key != "host_photo":                # the hooks build against the product
            bad = first_mismatch(got["product:" + case + ".bytes"], got[case + ".bytes"], 16)
            assert bad is None, (name, key, st, case, "product library differs from the hooks build", bad)

    # route: every call's witness against the tables
    for case, _, _, _, _ in child.device_cases():
        expect = _device_expected(device_table, case)
        assert np.array_equal(got[case + ".ctr"], expect), (name, case, "counted", _named(got[case + ".ctr"]), "expected", _named(expect))
    shapes = HOST[host_table][1]
    calls = {st: 0 for st in child.HOST_PROFILES}
    for case, st, dst_dev in child.host_cases():
        allowed = shapes["device_dst"] if dst_dev else shapes[st][calls[st]]
        if not dst_dev:
            calls[st] += 1
        expect = _host_expected(host_table, st, allowed)
        assert any(np.array_equal(got[case + ".ctr"], e) for e in expect), (name, case, "counted", _named(got[case + ".ctr"]), "expected one of",
                                                                             [_named(e) for e in expect])
