"""mphip_intpol_met in the reference-rounding build (lib/libmptrac_hip_exact.so): every case of tests/intpol_cases.py
against the oracle's scalar calls, bit for bit, as tests/test_gpu_intpol.py asks of the default library -- the call's
definition names IEEE operations that neither build contracts or replaces.  A process loads one of the two libraries, so
the census runs in a child with MPTRAC_AMD_EXACT=1; the SHA-256 of all bytes it returns is then compared with that of the
default library in this process."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys
sys.path[:0] = [ROOT, ROOT + "/tests"]
from mptrac_amd import hip
import test_gpu_intpol as T
print("library:", hip.load().mphip_version().decode())
wrong, digest = T.census()
print("JSON " + json.dumps({"wrong": wrong, "digest": digest}))
""".replace("ROOT", repr(ROOT))


def test_reference_rounding_build_gives_the_oracles_bits_and_the_default_library_the_same_bytes():
    env = dict(os.environ, MPTRAC_AMD_EXACT="1")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert "reference rounding" in lib, lib
    row = [json.loads(ln[5:]) for ln in res.stdout.splitlines() if ln.startswith("JSON ")][0]
    assert row["wrong"] == [], row["wrong"][:5]
    # the default library, here
    import test_gpu_intpol as T
    from mptrac_amd import hip
    assert "reference rounding" not in hip.load().mphip_version().decode()
    wrong, digest = T.census()
    assert wrong == [] and digest == row["digest"]
