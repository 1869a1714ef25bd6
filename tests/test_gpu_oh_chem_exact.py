"""module_oh_chem in the reference-rounding build (lib/libmptrac_hip_exact.so) against tests/refchem.py in the C
library's arithmetic: bit for bit without the diurnal scaling of OH (OH_CHEM_BETA 0); with it, the OH value carries the
device's trigonometry of the solar zenith angle (as module_meteo's oh quantity does) and agrees to 1e-12.  A process loads one of the two libraries, so the comparison runs in a child with
MPTRAC_AMD_EXACT=1 (as tests/test_gpu_exact_library.py does)."""
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
import test_gpu_oh_chem as T
print("library:", hip.load().mphip_version().decode())
for coord_type in (0, 1):
    for beta in (0.0, 0.6):
        for mix, (reaction, c) in enumerate(T.MIXES):
            g, ref, dt, atm = T.single_module(coord_type, beta, reaction, c, mode="libm")
            diff = int(np.sum(g["q"].view(np.uint64) != ref.view(np.uint64)))
            print("JSON " + json.dumps({"coord_type": coord_type, "beta": beta, "mix": mix, "differing": diff,
                                        "err": max(T.errors(g, ref, atm)),
                                        "acted": int(np.sum(g["q"][0] != atm["q"][0]))}))
""".replace("ROOT", repr(ROOT))


def test_reference_rounding_build_has_refchems_libm_bits():
    env = dict(os.environ, MPTRAC_AMD_EXACT="1")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert "reference rounding" in lib, lib
    rows = [json.loads(ln[5:]) for ln in res.stdout.splitlines() if ln.startswith("JSON ")]
    assert len(rows) == 32
    for r in rows:
        assert r["acted"] > 1000, r
        if r["beta"] == 0:
            assert r["differing"] == 0, r
        else:      # (the solar zenith angle of clim_oh: the device library's sin / cos / atan2, as in module_meteo)
            assert r["err"] <= 1e-12, r
