"""The axis-search edge inputs (tests/axis_cases.py) in the reference-rounding build (lib/libmptrac_hip_exact.so): the
single modules at the exact positions on every warped grid and one 20-step run, through the functions of
tests/test_gpu_axis_edges.py with tolerance 0 -- positions, quantities and cache->uvwp by array_equal with the oracle,
which is that library's contract.  There locate_lon is locate_reg, so a particle on a grid line takes the reference's
cell, not the neighbouring one with the same interpolated value.  A process loads one of the two libraries, so the
comparison runs in a child with MPTRAC_AMD_EXACT=1."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
sys.path[:0] = [ROOT, ROOT + "/tests"]
from mptrac_amd import hip
import test_gpu_axis_edges as T
print("library:", hip.load().mphip_version().decode())
one_degree = sys.argv[1] == "C1"
for combo in T.COMBOS:
    if (combo[0] == "C1") == one_degree:
        for case in T.GROUPS:
            T.single_modules(case, combo, tol=0.0)
for combo in T.RUNS[:2]:
    if (combo[0] == "C1") == one_degree:
        T.whole_run("conv_sedi", combo, tol=0.0)
""".replace("ROOT", repr(ROOT))


@pytest.mark.parametrize("grid", ["36x19x40", "C1"])
def test_reference_rounding_build_has_the_oracles_bits_on_the_grid_lines(grid):
    env = dict(os.environ, MPTRAC_AMD_EXACT="1")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, "-c", CHILD, grid], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert "reference rounding" in lib, lib
    rows = [json.loads(ln[10:]) for ln in res.stdout.splitlines() if ln.startswith("AXIS_EDGE ")]
    n_combos = 4 if grid == "C1" else 12
    assert len([r for r in rows if r["test"] == "single"]) == n_combos * 11 and len([r for r in rows if r["test"] == "run"]) == 2
    for r in rows:
        assert r["lon"] == 0 and r["lat"] == 0 and r["p"] == 0 and r["q"] == 0 and r["uvwp"] and r["time"], r
