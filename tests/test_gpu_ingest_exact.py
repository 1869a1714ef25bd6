"""mphip_ingest_met in the reference-rounding build (lib/libmptrac_hip_exact.so): the census of tests/test_gpu_ingest.py --
every case of tests/ingest_cases.py in one call, into strided views, stage by stage, in two calls and in place --, the
refusals and the call from a second thread, against tests/refingest.py bit for bit, as in the default library: the
definition names IEEE operations that neither build contracts or replaces.  A process loads one of the two libraries, so
the census runs in a child with MPTRAC_AMD_EXACT=1; its bytes are then compared with those the default library returns in
this process."""
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
import test_gpu_ingest as T
print("library:", hip.load().mphip_version().decode())
sim = T.bare_context()
wrong, digest = T.census(sim)
refusals = [[name, rc, msg, bool(kept), expect] for name, rc, msg, kept, expect in T.refusal_rows(sim)]
sim.close()
errors, good, same = T.second_thread()
print("JSON " + json.dumps({"wrong": wrong, "digest": digest, "refusals": refusals, "thread": [errors, bool(good), bool(same)]}))
""".replace("ROOT", repr(ROOT))


def test_reference_rounding_build_gives_the_restatement_bits_and_the_default_library_the_same_bytes():
    env = dict(os.environ, MPTRAC_AMD_EXACT="1")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert "reference rounding" in lib, lib
    row = [json.loads(ln[5:]) for ln in res.stdout.splitlines() if ln.startswith("JSON ")][0]
    assert row["wrong"] == [], row["wrong"][:5]
    import test_gpu_ingest as T
    assert len(row["refusals"]) == 2 * T.N_REFUSALS
    for name, rc, msg, kept, expect in row["refusals"]:
        if expect:
            assert rc != 0 and msg == expect and kept, (name, rc, msg, kept)
        else:
            assert msg == "", (name, msg)
    assert row["thread"] == [[], True, True], row["thread"]
    # the default library, here
    from mptrac_amd import hip
    assert "reference rounding" not in hip.load().mphip_version().decode()
    sim = T.bare_context()
    try:
        wrong, digest = T.census(sim)
    finally:
        sim.close()
    assert wrong == [] and digest == row["digest"]
