"""Backward runs in the reference-rounding build (lib/libmptrac_hip_exact.so): every named case 20 steps backward, the
two-hour hand-over runs and the staggered releases of tests/test_gpu_backward.py through the same functions with
tolerance 0 -- after the last step (and behind every hand-over) positions, every quantity row and cache->uvwp are the
oracle's bits.  No row is left out: the forward census (tests/test_gpu_exact_library.py) leaves none out either -- the
cell sums of module_mixing add in the order of the particle index on both sides.  A process loads one of the two
libraries, so the comparison runs in a child with MPTRAC_AMD_EXACT=1."""
import json
import os
import subprocess
import sys

import pytest

import cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys, traceback
sys.path[:0] = [ROOT, ROOT + "/tests"]
from mptrac_amd import hip
import test_gpu_backward as T
print("library:", hip.load().mphip_version().decode())
failed = 0
for arg in sys.argv[2:]:
    try:
        if sys.argv[1] == "named":
            T.named_case(arg, tol=0.0)
        elif sys.argv[1] == "handover":
            T.handover(arg, 2, tol=0.0)
        else:
            case, _, sort = arg.partition(":")
            T.staggered(case, tol=0.0, **(dict(sort_dt=0.0) if sort == "unsorted" else {}))
    except AssertionError:
        failed += 1
        print("FAILED", arg)
        traceback.print_exc(file=sys.stdout)
sys.exit(1 if failed else 0)
""".replace("ROOT", repr(ROOT))

_NAMES = list(cases.CASES)
GROUPS = [("named", _NAMES[0::3]), ("named", _NAMES[1::3]), ("named", _NAMES[2::3]),
          ("handover", ["diff", "full", "zeta_full", "mlp_full", "bound_pbl_zeta", "meteo", "meteo_gated"]),
          ("staggered", ["conv_sedi", "full", "full:unsorted"])]


@pytest.mark.parametrize("what,args", GROUPS, ids=["named_0", "named_1", "named_2", "handover_2h", "staggered"])
def test_reference_rounding_build_has_the_oracles_bits_backward(what, args):
    env = dict(os.environ, MPTRAC_AMD_EXACT="1")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, "-c", CHILD, what, *args], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert "reference rounding" in lib, lib
    rows = [json.loads(ln[9:]) for ln in res.stdout.splitlines() if ln.startswith("BACKWARD ")]
    assert [r["case"] for r in rows] == [a.partition(":")[0] for a in args]
    for r in rows:
        assert r["time"] and r["uvwp"] and r["lon"] == r["lat"] == r["p"] == r["q_bits"] == 0 and r["pos"] == r["q"] == 0.0, r
