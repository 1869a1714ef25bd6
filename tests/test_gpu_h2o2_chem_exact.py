"""module_chem_grid and module_h2o2_chem in the reference-rounding build (lib/libmptrac_hip_exact.so) against
tests/refh2o2.py in the C library's arithmetic: Cx and every quantity bit for bit.  The diurnal scaling of OH stays off
(tests/test_gpu_oh_chem_exact.py: it carries the device's trigonometry).  A process loads one of the two libraries, so
the comparison runs in a child with MPTRAC_AMD_EXACT=1."""
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
import test_gpu_h2o2_chem as T
print("library:", hip.load().mphip_version().decode())
for names in T.H2O2_SETS:
    g, ref, dt, atm, f = T.single_h2o2(names, mode="libm", nens=3 if "ens" in names else 0)
    diff = int(np.sum(g["q"].view(np.uint64) != ref.view(np.uint64)))
    print("JSON " + json.dumps({"module": "h2o2", "names": names, "differing": diff,
                                "acted": int(np.sum(g["q"] != atm["q"]))}))
for grid, nens, names in ((T.GRID, 0, ("m", "vmr", "Cx")), (T.DEFAULT_GRID, 0, ("m", "Cx")), (T.GRID, 4, ("m", "Cx", "ens"))):
    g, ref, cell, atm = T.single_grid(names, mode="libm", grid=grid, nens=nens)
    diff = int(np.sum(g["q"].view(np.uint64) != ref.view(np.uint64)))
    print("JSON " + json.dumps({"module": "chem_grid", "names": names, "differing": diff,
                                "acted": int(np.sum(cell >= 0))}))
""".replace("ROOT", repr(ROOT))


def test_reference_rounding_build_has_refh2o2s_libm_bits():
    env = dict(os.environ, MPTRAC_AMD_EXACT="1")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert "reference rounding" in lib, lib
    rows = [json.loads(ln[5:]) for ln in res.stdout.splitlines() if ln.startswith("JSON ")]
    assert len(rows) == 9
    for r in rows:
        assert r["acted"] > 300, r
        assert r["differing"] == 0, r
