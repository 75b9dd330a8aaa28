"""No environment switch of the library goes unlisted: every "ITW_..." string literal in csrc/*.hip and csrc/*.hpp is either a row variable
of tests/test_gpu_launch_switches.py (run in a fresh process each, with a route witness) or named in COVERED_ELSEWHERE with the place that
exercises it -- or with the reason it selects no encode route.  A new switch fails this test until someone decides where it is tested."""
import glob
import os
import re

from test_gpu_launch_switches import ROW_VARIABLES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "intel-texture-works-plugin_amd", "csrc")

# name -> (file that exercises it, what that file must contain, a line for the reader); file None: no route to test, and why
COVERED_ELSEWHERE = {
    # read at every call: compared in one process
    "ITW_BC7_PAIRS":        ("tests/test_gpu_bc7_pairs.py", "ITW_BC7_PAIRS", "every route against the oracle; also a per-call knob of the launch-switch child"),
    "ITW_BC7_PAIR_CAP":     ("tests/test_gpu_bc7_pairs.py", "ITW_BC7_PAIR_CAP", "the overflow route"),
    "ITW_BC7_ROT_TASKS":    ("tests/test_gpu_bc7_rot_tasks.py", "ITW_BC7_ROT_TASKS", "both rotation routes against the oracle"),
    "ITW_HOST_RUNS":        ("tests/test_gpu_host_runs_small.py", "ITW_HOST_RUNS", "the staged runs at their smallest size; the cut itself in tests/test_host_runs_cpu.py"),
    "ITW_HOST_CHUNKS":      ("tests/test_gpu_host_runs_small.py", "ITW_HOST_CHUNKS", "equal runs of a PCIe-bound format"),
    # switches with a setter: the setter is what the tests drive
    "ITW_BC7_PILOT_THR":    ("tests/test_gpu_bc7_pairs_in_finish.py", "pilots=", "itwSetBc7Pilot overrides it: both verdicts forced in-process; the child here calls the setter too"),
    "ITW_BC6H_PATH":        ("tests/test_gpu_bc7_paths.py", "test_bc6h_wide_at_every_split_width", "itwSetBc7Path sets the BC6H path with the BC7 one"),
    "ITW_SLICE_WINDOW":     ("tests/test_dispatch_layer.py", "ITW_SLICE_WINDOW", "itwSetSliceWindow; the variable's reading in tests/test_host_geometry_cpu.py"),
    "ITW_SLICED_PIPELINE":  ("tests/test_dispatch_layer.py", "ITW_SLICED_PIPELINE", "itwSetSliceWindow(-1) is the same setting"),
    "ITW_ON_ERROR":         ("tests/test_abi_boundary.py", "ON_ERROR_RETURN", "itwSetErrorMode: how a failure is reported, no encode route"),
    "ITW_MULTIGPU_INTERLEAVE": ("tests/test_gpu_multigpu_cpp.py", "itwMultiGpuSetInterleave", "the setter"),
    "ITW_WORKERS":          ("tests/test_dispatch_layer.py", "ITW_WORKERS", "the dispatch layer's pool size"),
    "ITW_MULTIGPU_POST_TIMEOUT_S": ("tests/test_gpu_multigpu_cpp.py", "ITW_MULTIGPU_POST_TIMEOUT_S", "the watchdog, in a child process"),
    # no encode route behind them
    "ITW_MULTIGPU_TIMEOUT_S":      (None, None, "a watchdog limit: no encode route"),
    "ITW_MULTIGPU_INIT_TIMEOUT_S": (None, None, "a watchdog limit: no encode route"),
    "ITW_MULTIGPU_AFFINITY":       (None, None, "host thread placement: no encode route"),
    "ITW_MULTIGPU_TRANSPORT":      (None, None, "how finished bands travel between GPUs: needs several GPUs, no encode route"),
    "ITW_MULTIGPU_RANKS":          (None, None, "the rank count of a multi-GPU call that names none: needs several GPUs, no single-GPU encode route"),
    "ITW_COALESCE_DEBUG":   (None, None, "a report at exit; the hooks build counts always (tests/test_gpu_call_combiner.py)"),
    "ITW_COALESCE":         (None, None, "combiner off: every call then takes the route a lone call takes, which is what the other tests run"),
    "ITW_BC7_PILOT_DEBUG":  ("tests/test_gpu_bc7_pairs_in_finish.py", "ITW_BC7_PILOT_DEBUG", "prints counters, in a child process; chooses nothing"),
    "ITW_SLICE_LOOKAHEAD":  (None, None, "how many windows are issued ahead: timing only, the same launches in the same order per stream"),
    # too large for a per-row child: said so
    "ITW_BC7_WINDOW_MIN":   (None, None, "from which size a host-pointer BC7 call takes windows: 0 cannot lower it below two windows of 131 072 blocks "
                                         "(about 196 608 blocks in all), too large for a per-row child; tests/test_gpu_host_pointer_runs.py runs the windows at 2048 x 4096"),
    "ITW_HOST_WINDOWS_OFF": (None, None, "keeps such a call on the staged runs: the same size; the staged runs themselves are tests/test_gpu_host_runs_small.py's"),
}


def _literals():
    names = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp"))):
        with open(path) as f:
            names |= set(re.findall(r'"(ITW_[A-Z0-9_]+)"', f.read()))
    return names


def test_every_switch_is_a_row_or_listed():
    names = _literals()
    assert len(names) >= 30 and "ITW_BC7_COMPACT" in names and "ITW_STAGED_WIDE_MAX" in names, sorted(names)      # the scan found the sources
    unlisted = sorted(n for n in names if n not in ROW_VARIABLES and n not in COVERED_ELSEWHERE)
    assert not unlisted, f"{unlisted}: add a row to tests/test_gpu_launch_switches.py or an entry to COVERED_ELSEWHERE"
    gone = sorted(n for n in list(ROW_VARIABLES) + list(COVERED_ELSEWHERE) if n not in names)
    assert not gone, f"{gone}: listed here, read nowhere in csrc/"


def test_every_row_variable_is_read_once_per_process():
    """what the issue's matrix is for: none of them is in the table of switches read at every call"""
    assert set(ROW_VARIABLES) == {"ITW_BC7_PATH", "ITW_BC7_FUSED", "ITW_BC7_BOUND", "ITW_BC7_ALPHA_PRUNE", "ITW_BC7_BANDS", "ITW_BC7_COMPACT",
                                  "ITW_STAGED_BANDS", "ITW_STAGED_VERDICT_THR", "ITW_STAGED_WIDE_MAX"}
    assert not set(ROW_VARIABLES) & set(COVERED_ELSEWHERE)


def test_every_named_file_exists_and_names_it():
    for name, (path, needle, why) in COVERED_ELSEWHERE.items():
        assert why, name
        if path is None:
            continue
        full = os.path.join(ROOT, path)
        assert os.path.isfile(full), (name, path)
        with open(full) as f:
            assert needle in f.read(), (name, path, needle)
