"""The driver's contract with bench.py, on the GPU: `python bench.py --gpus 1 --steps K --warmup W` prints ONE JSON line with the
keys the driver and the judge read (metric / value / unit / n_gpus / steps / warmup / ms_per_step / higher_is_better / scaling /
vs_baseline / dtype / data / config.workload), K steps were timed and nothing else ran, and --dump-outputs writes the stream of the
last step; with --full the line also has a `roofline` object for the dominant kernel and a `cpu_baseline` object, and the numbers
are consistent with each other."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_json_line_with_the_contract_keys(gpu):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-formats", "--full"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 3 and j["warmup"] == 1 and j["higher_is_better"] is True and j["unit"] == "Mpixels/s"
    assert j["dtype"] == "f32" and j["data"] == "synthetic" and j["vs_baseline"] is None and "workload" in j["config"]
    assert "4096x4096" in j["config"]["workload"] and "BC7 GetProfile_slow" in j["config"]["workload"]        # BASELINE configs[2]
    # value = pixels per step / time per step
    assert abs(j["value"] - 4096 * 4096 / (j["ms_per_step"] * 1e-3) / 1e6) / j["value"] < 1e-3
    rf = j["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["unit"] == "GB/s" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-4 and rf["hbm_frac"] == rf["frac"]
    assert j["abi_calls"] == 3 + 1 + 1 + 3                    # timed + warm-up steps, then the HIP-event leg's warm-up + launches
    # The binding roofline as scalars: present whenever the committed counter pass was taken on these kernel sources.
    # BC7 is VALU-issue bound; `frac` stays the contract's HBM fraction and says so.
    if rf.get("profile_matches_source", {}).get("valu"):
        assert rf["bound"] == "valu-issue" and 0 < rf["valu_frac"] <= 1.0 and rf["valu_frac"] == rf["valu"]["frac"] and "frac_is" in rf
        assert rf["issue_frac"] is None or 0 < rf["issue_frac"] <= 1.05
        iso = rf["rocprof_kernels"]["isolated"]
        # serialised per-kernel durations: their sum cannot be below the overlapped call (two bands on two streams)
        assert iso["sum_ms"] >= rf["kernel_ms_avg"] * 0.97 and all(0 <= k["lane_op_frac"] <= 1.0 for k in iso["kernels"].values())
        assert abs(sum(k["wave_valu"] for k in iso["kernels"].values()) - rf["valu"]["wave_instructions_per_call"]) <= 0.02 * rf["valu"]["wave_instructions_per_call"]
    else:
        assert rf["bound"] == "hbm"
    assert rf["algorithmic_bytes_per_launch"] == 80 * (4096 // 4) ** 2
    assert 0 < rf["kernel_ms_avg"] <= j["ms_per_step"] * 1.05                     # the kernels of a step fit inside the step
    if "valu" in rf:
        assert 0 < rf["valu"]["frac"] <= 1.0
    va = rf.get("valu_algorithmic")
    if va:
        # never a key that reads as a roofline fraction; the reference-equivalent rate itself may exceed the peak since the
        # bounded mode order skips work exactly (round 4)
        assert "frac" not in va and "frac_of_fma_peak" not in va and va["reference_equivalent_over_fma_peak"] > 0
    cb = j["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] in ("reference", "port") and cb["cores"] >= 1 and cb["value"] > 0


def test_plain_run_times_the_steps_and_dumps_the_last_one(itw, gpu, tmp_path):
    """A plain run is lean: the headline keys, exactly K timed steps after W warm-up steps and no other encode call (abi_calls), none of
    the --full figures; --dump-outputs holds the whole 4096^2 BC7 `slow` stream of the last step (float32 16-bit words), which is what
    the library gives for the same seeded surface in this process."""
    import numpy as np
    import torch
    import bench
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--dump-outputs", d],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "config"):
        assert k in j, k
    assert j["steps"] == 4 and j["warmup"] == 2 and j["abi_calls"] == 4 + 2 and j["unit"] == "Mpixels/s" and j["higher_is_better"] is True
    assert "4096x4096" in j["config"]["workload"] and "BC7 GetProfile_slow" in j["config"]["workload"]
    assert abs(j["value"] - 4096 * 4096 / (j["ms_per_step"] * 1e-3) / 1e6) / j["value"] < 1e-3
    assert not {"roofline", "formats", "cpu_baseline"} & set(j), sorted(j)
    a = np.load(os.path.join(d, "blocks.npy"))
    assert a.dtype == np.float32 and a.shape == ((4096 // 4) ** 2, 8) and not os.path.exists(os.path.join(d, "block_index.npy"))
    got = np.ascontiguousarray(a.astype("<u2")).view(np.uint8).reshape(-1)
    want = itw.compress("bc7", torch.from_numpy(bench.make_surface("bc7", 4096, 0)).to(gpu), "slow")
    torch.cuda.synchronize()
    assert np.array_equal(got, want.cpu().numpy().reshape(-1))
