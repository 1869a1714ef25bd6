"""module_radio_decay in the reference-rounding build (lib/libmptrac_hip_exact.so) against tests/refradio.py in the C
library's arithmetic (exp): bit for bit (tolerance 0) -- the decay constants are folded at compile time, exp is the
glibc-exact one, no multiply-add is contracted and the Pb-210 expression has the restatement's association.  A process
loads one of the two libraries, so the comparison runs in a child with MPTRAC_AMD_EXACT=1."""
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
import test_gpu_radio_decay as T
print("library:", hip.load().mphip_version().decode())
for names, steps, direction in ((T.ACT, 1, 1), (("m",) + T.ACT + ("vmr",), 20, 1), (("Apb210", "m", "Arn222"), 3, -1),
                                (("Apb210",), 1, 1)):
    g, ref, dt, atm = T.single(names, mode="libm", n=20000, steps=steps, direction=direction)
    rows = [k for k, x in enumerate(names) if x in T.ACT]
    bits = all(np.array_equal(g["q"][k], ref[k]) for k in rows)
    err = max(T.rel(g["q"][k], ref[k]) for k in rows)
    kept = all(np.array_equal(g["q"][k], atm["q"][k]) for k in range(len(names)) if k not in rows)
    print("JSON " + json.dumps({"names": names, "steps": steps, "direction": direction, "bits": bits, "err": err,
                                "kept": kept, "acted": int(np.sum(g["q"][rows] != atm["q"][rows]))}))
""".replace("ROOT", repr(ROOT))


def test_reference_rounding_build_gives_the_libm_restatement_bits():
    env = dict(os.environ, MPTRAC_AMD_EXACT="1")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert "reference rounding" in lib, lib
    rows = [json.loads(ln[5:]) for ln in res.stdout.splitlines() if ln.startswith("JSON ")]
    assert len(rows) == 4
    for r in rows:
        assert r["acted"] > 10000, r
        assert r["kept"], r
        assert r["bits"] and r["err"] == 0.0, r
