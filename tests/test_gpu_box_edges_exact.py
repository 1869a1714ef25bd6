"""The box-edge inputs (tests/box_cases.py) in the reference-rounding build (lib/libmptrac_hip_exact.so), through the
functions of tests/test_gpu_box_edges.py with tolerance 0 wherever that library's contract reaches: module_mixing and
the gridded output with ordered sums, the CSI and profile boxes, the chemistry grid against the reference in the C
library's arithmetic, and the time steps of the three producers -- positions, quantities and sums by array_equal.  The
atomic sums add in the order of arrival in either build and keep their bar.  A process loads one of the two libraries,
so the comparison runs in a child with MPTRAC_AMD_EXACT=1."""
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
import box_cases as BC
import test_gpu_box_edges as T
print("library:", hip.load().mphip_version().decode())
for name in BC.GRIDS:
    for nens in (0, BC.NMEMBER):
        T.mixing_ordered(name, nens)
        T.mixing_atomics(name, nens)
    T.gridded(name, exact=True)
for name in ("A", "B"):
    T.box_sums(name)
T.chem_grid(exact=True)
T.producers(tol=0.0)
""".replace("ROOT", repr(ROOT))


def test_reference_rounding_build_has_the_references_cells_and_bits():
    env = dict(os.environ, MPTRAC_AMD_EXACT="1")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert "reference rounding" in lib, lib
    rows = [json.loads(ln[9:]) for ln in res.stdout.splitlines() if ln.startswith("BOX_EDGE ")]
    by = {}
    for r in rows:
        by.setdefault(r["test"], []).append(r)
    # grids x members x orders x algorithms; grids x orders x algorithms x value sources; two boxes x orders x paths
    assert {k: len(v) for k, v in by.items()} == {"mixing": 32, "mixing_atomics": 8, "gridded": 32, "gridded_weighted": 32,
                                                  "box_sums": 12, "chem_grid": 1, "producers_oracle": 2,
                                                  "producers_equal": 2}
    assert all(r["differing"] == 0 for r in by["mixing"])
    assert all(r["err"] <= 1e-12 and r["flip_margin"] > 1e-6 for r in by["mixing_atomics"])
    assert all(all(r["equal"]) for r in by["gridded"] + by["box_sums"])
    assert all(r["counts"] and r["equal"] for r in by["gridded_weighted"])
    assert by["chem_grid"][0]["differing"] == 0
    for r in by["producers_oracle"]:
        assert r["lon"] == 0 and r["lat"] == 0 and r["p"] == 0 and r["q"] == 0 and r["uvwp"] and r["time"], r
    for r in by["producers_equal"]:
        assert all(v for k, v in r.items() if k not in ("test", "grid", "emit_keys", "ahead_box")), r
