"""mphip_select_atm in the reference-rounding build (lib/libmptrac_hip_exact.so), through the functions of
tests/test_gpu_select.py: the same comparisons, array_equal everywhere -- both libraries decide alike and return the bits
mphip_get_atm has.  A process loads one of the two libraries, so the comparison runs in a child with MPTRAC_AMD_EXACT=1."""
import json
import os
import subprocess
import sys

import pytest

import select_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
sys.path[:0] = [ROOT, ROOT + "/tests"]
from mptrac_amd import hip
import select_cases as SC
import test_gpu_select as T
print("library:", hip.load().mphip_version().decode())
for name in SC.set_names():
    for variant in SC.variants_of(name):
        T.every_call(name, variant)
T.steps_with_calls_in_between()
T.refusals()
T.one_rank_of_two()
""".replace("ROOT", repr(ROOT))


def test_reference_rounding_build_selects_the_same_particles():
    env = dict(os.environ, MPTRAC_AMD_EXACT="1")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert "reference rounding" in lib, lib
    rows = [json.loads(ln[7:]) for ln in res.stdout.splitlines() if ln.startswith("SELECT ")]
    assert all(r["equal"] for r in rows)
    per_set = {}
    for r in rows:
        if r.get("set") and "reference" in r and r.get("cap") is None:
            per_set.setdefault((r["set"], r["variant"]), []).append(r)
    for name in SC.set_names():
        for variant in SC.variants_of(name):
            for path in ("", "/direct"):
                assert len(per_set[(name, variant + path)]) == len(SC.calls_of(name)), (name, variant + path)
    assert sum(r["reference"] for v in per_set.values() for r in v) > 100000
    assert any(r.get("test") == "stepping" for r in rows) and sum(r.get("test") == "refusal" for r in rows) >= 16
