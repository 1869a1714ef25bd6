"""module_tracer_chem in the reference-rounding build (lib/libmptrac_hip_exact.so) against tests/reftracer.py in the C
library's arithmetic (exp, acos), within 1e-12: not bit for bit, because the solar zenith angle (cos_sza's
trigonometry, acos) is the device's own -- the reason the diurnal OH case is held to 1e-12 too
(tests/test_gpu_oh_chem_exact.py).  A process loads one of the two libraries, so the comparison runs in a child with
MPTRAC_AMD_EXACT=1."""
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
import test_gpu_tracer_chem as T
print("library:", hip.load().mphip_version().decode())
for names in (T.SPECIES, ("m",) + T.SPECIES + ("Csf6",)):
    g, ref, dt, atm, f = T.single(names, mode="libm", n=20000)
    rows = [k for k, x in enumerate(names) if x in T.SPECIES]
    err = max(T.rel(g["q"][k], ref[k]) for k in rows)
    kept = all(np.array_equal(g["q"][k], atm["q"][k]) for k in range(len(names)) if k not in rows)
    print("JSON " + json.dumps({"names": names, "err": err, "kept": kept,
                                "acted": int(np.sum(g["q"][rows] != atm["q"][rows]))}))
""".replace("ROOT", repr(ROOT))


def test_reference_rounding_build_against_the_libm_restatement():
    env = dict(os.environ, MPTRAC_AMD_EXACT="1")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert "reference rounding" in lib, lib
    rows = [json.loads(ln[5:]) for ln in res.stdout.splitlines() if ln.startswith("JSON ")]
    assert len(rows) == 2
    for r in rows:
        assert r["acted"] > 40000, r
        assert r["kept"], r
        assert r["err"] <= 1e-12, r
