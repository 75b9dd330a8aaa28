"""bc7_bound_list exists because the 64 two-subset bounds are an ALU-only chain that ran, inside bc7_finish_all<10>, at the two waves per SIMD the
refinement's palette LDS allows.  This test reads the built code object (tools/kernel_resources.py over csrc/build/bc7.o) and holds what that
move rests on: the new kernel keeps its registers (no spilled VGPRs, no scratch), has only the claim's LDS, and reaches the waves per SIMD it was
tuned for under both limits (512 registers per SIMD lane, 160 KiB of LDS per CU; 256-lane workgroups: one wave per SIMD each); PHASE 10, without
the tail and with mode 6's 16-level palette, holds the waves chosen for it; the refinement phases before and behind them stay at two.
The tuned values are the measured ones: profiles/r11_bc7_insts_valu.txt (the wave settings tried, with their times)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "intel-texture-works-plugin_amd", "csrc", "build", "bc7.o")

BOUND_LIST_WAVES = 6          # amdgpu_waves_per_eu of bc7_bound_list (BOUND_LIST_WAVES in csrc/bc7.hip)
WAVES = {"bc7_bound_list<true>": BOUND_LIST_WAVES, "bc7_bound_list<false>": BOUND_LIST_WAVES,
         "bc7_finish_all<true, 10>": 3, "bc7_finish_all<true, 9>": 2, "bc7_finish_all<true, 8>": 2}


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(OBJ):
        pytest.skip("csrc/build/ is not populated: run __graft_entry__.build() first")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), OBJ], check=True, capture_output=True, text=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"(?:void )?itw::(\S.*?)\s+vgpr\s+(\d+) agpr\s+(\d+) sgpr\s+\d+ scratch\s+(\d+) B\s+lds\s+(\d+) B\s+spills v(\d+) s(\d+)", line)
        if m:
            rows[m.group(1)] = dict(regs=int(m.group(2)) + int(m.group(3)), scratch=int(m.group(4)), lds=int(m.group(5)), vspill=int(m.group(6)))
    return rows


def waves(row):
    by_regs = 512 // (-(-row["regs"] // 8) * 8)
    by_lds = (160 * 1024) // row["lds"] if row["lds"] else 8
    return min(by_regs, by_lds, 8), by_regs, by_lds


@pytest.mark.parametrize("name", sorted(WAVES))
def test_kernel_holds_the_waves_it_was_tuned_for(table, name):
    assert name in table, (name, sorted(table))
    got, by_regs, by_lds = waves(table[name])
    assert got == WAVES[name], f"{name}: {table[name]} -> {by_regs} waves by registers, {by_lds} by LDS; tuned for {WAVES[name]}"


@pytest.mark.parametrize("name", ["bc7_bound_list<true>", "bc7_bound_list<false>"])
def test_bound_list_keeps_its_registers_and_has_only_the_claims_lds(table, name):
    row = table[name]
    assert row["vspill"] == 0 and row["scratch"] == 0, row
    assert 0 < row["lds"] <= 2048, row
