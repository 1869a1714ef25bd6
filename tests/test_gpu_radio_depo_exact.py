"""module_radio_depo in the reference-rounding build (lib/libmptrac_hip_exact.so): the module alone and twenty steps with
everything on (tests 1 and 3 of tests/test_gpu_radio_depo.py) against tests/refradiodepo.py fed with the oracle's factors,
bit for bit -- activities and inventory by array_equal.  The factors are the oracle's exp / pow, the ground decay is the
C library's exp on the host, products and differences are rounded once, the sums add in ascending particle index.  A
process loads one of the two libraries, so the comparison runs in a child with MPTRAC_AMD_EXACT=1."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [ROOT, ROOT + "/tests"]
from mptrac_amd import hip
import test_gpu_radio_depo as T
print("library:", hip.load().mphip_version().decode())
for case in T.CASES:
    q, ref, dt_ref, fac = T.module_alone_reference(case)
    atm = T.inputs(case)[4]
    g, dt, inv = T.device_module_alone(case)
    assert np.array_equal(dt, dt_ref)
    T.check_against(g, inv, q, ref, atm, dt, 0)
    print("JSON " + json.dumps({"test": "alone", "case": case, "wet": float(inv[1].sum()), "dry": float(inv[2].sum())}))
clim, m0, m1, atm = T.inputs("full", n=T.TWENTY_N)[1:]
ctl, times, o, ref, history, _ = T.twenty_steps_reference("full", True, "libm")
for h in history[-3:]:
    T.assert_coverage(*h)
g, inv = T.device_twenty_steps(ctl, clim, m0, m1, atm, times)
T.check_twenty_steps(g, inv, o, ref, 0)
print("JSON " + json.dumps({"test": "twenty", "case": "full", "wet": float(inv[1].sum()), "dry": float(inv[2].sum())}))
""".replace("ROOT", repr(ROOT))


def test_reference_rounding_build_gives_the_restatement_bits():
    env = dict(os.environ, MPTRAC_AMD_EXACT="1")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert "reference rounding" in lib, lib
    rows = [json.loads(ln[5:]) for ln in res.stdout.splitlines() if ln.startswith("JSON ")]
    assert [r["test"] for r in rows] == ["alone", "alone", "twenty"]
    for r in rows:
        assert r["wet"] > 0 and r["dry"] > 0, r
