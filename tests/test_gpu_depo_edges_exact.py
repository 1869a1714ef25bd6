"""The decision-edge cases (tests/depo_cases.py) in the reference-rounding build (lib/libmptrac_hip_exact.so): the single
modules of every case and the time steps of every run in every launch shape, through the functions of
tests/test_gpu_depo_edges.py with tolerance 0 -- positions, quantities and cache->uvwp by
np.array_equal(..., equal_nan=True) with the oracle, which is that library's contract; where the oracle's value is not
finite (pct == pcb) the same bits.  A process loads one of the two libraries, so the comparison runs in a child with
MPTRAC_AMD_EXACT=1."""
import json
import os
import subprocess
import sys

import pytest

import depo_cases as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = sorted({n.split("-")[0] for n in D.all_cases()})

CHILD = r"""
import sys
sys.path[:0] = [ROOT, ROOT + "/tests"]
from mptrac_amd import hip
import test_gpu_depo_edges as T
print("library:", hip.load().mphip_version().decode())
what = sys.argv[1]
if what.startswith("run:"):
    T.time_steps(what[4:], tol=0.0)
else:
    for name in T.NAMES:
        if name.split("-")[0] == what:
            T.single_modules(name, tol=0.0)
""".replace("ROOT", repr(ROOT))


@pytest.mark.parametrize("what", FAMILIES + ["run:" + w for w in ("behind_mixing", "fused_tail", "extrap_run-east", "extrap_run-west")])
def test_reference_rounding_build_has_the_oracles_bits_at_the_decision_edges(what):
    env = dict(os.environ, MPTRAC_AMD_EXACT="1")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, "-c", CHILD, what], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert "reference rounding" in lib, lib
    rows = [json.loads(ln[10:]) for ln in res.stdout.splitlines() if ln.startswith("DEPO_EDGE ")]
    if what.startswith("run:"):
        assert len(rows) == (9 if "extrap" in what else 10), len(rows)
    else:
        assert len(rows) == sum(len(c["modules"]) for n, c in D.all_cases().items() if n.split("-")[0] == what), len(rows)
    for r in rows:
        assert r["lon"] == 0 and r["lat"] == 0 and r["p"] == 0 and r["q"] == 0 and r["device_only"] == 0 and r["oracle_only"] == 0, r
