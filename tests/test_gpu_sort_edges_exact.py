"""The placed sort cases (tests/sort_cases.py) in the reference-rounding build (lib/libmptrac_hip_exact.so): one case per
pass plan, the all-equal keys, and the repairs with no mover, with movers only and with 4096 and then 4097 movers,
through the functions of tests/test_gpu_sort_edges.py with tolerance 0 -- positions by array_equal with the oracle, which
is that library's contract.  A process loads one of the two libraries, so the comparison runs in a child with
MPTRAC_AMD_EXACT=1."""
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
import sort_cases as S
import test_gpu_sort_edges as T
print("library:", hip.load().mphip_version().decode())
if sys.argv[1] == "scratch":
    for grid in S.GRIDS:
        T.scratch((grid, "tied", 4097, 0))
    T.scratch(("p2b8", "equal_first", 8193, 0))
    T.scratch(("p1b9", "equal_last", 4097, 0))
else:
    for name in ("cross4096", "none", "all"):
        T.repair(name, tol=0.0)
""".replace("ROOT", repr(ROOT))


@pytest.mark.parametrize("part", ["scratch", "repair"])
def test_reference_rounding_build_sorts_and_repairs_the_placed_cases(part):
    env = dict(os.environ, MPTRAC_AMD_EXACT="1")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, "-c", CHILD, part], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert "reference rounding" in lib, lib
    rows = [json.loads(ln[10:]) for ln in res.stdout.splitlines() if ln.startswith("SORT_EDGE ")]
    if part == "scratch":
        assert len(rows) == 9 and {r["passes"] for r in rows} == {1, 2, 3} and {r["bits"] for r in rows} == {8, 9, 10}
        assert all(r["keys"] and r["perm"] and r["oracle"] and r["again"] for r in rows), rows
    else:
        assert len(rows) == 12 and [r["movers"] for r in rows if r["case"] == "cross4096"] == [0, 0, 4096, 4097]
        for r in rows:
            assert r["keys_on"] and r["perm_on"] and r["counts"] == [r["step"], 1], r
            assert r["oracle"] == {"lon": 0.0, "lat": 0.0, "p": 0.0} and all(r["oracle_exact"].values()), r
