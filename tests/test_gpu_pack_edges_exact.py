"""The edge cases of the 16-bit packed level fields in the reference-rounding build (lib/libmptrac_hip_exact.so):
tests/test_gpu_pack_edges.py's edge_census and the 257 x 241 x 137 grid (three passes of the streaming kernels) against
tests/refpack.py, bit for bit, as in the default library.  A process loads one of the two libraries, so the census runs in a
child with MPTRAC_AMD_EXACT=1; its bytes are then compared with those the default library returns in this process."""
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
import test_gpu_pack_edges as T
print("library:", hip.load().mphip_version().decode())
sim = T.bare_context()
wrong, digest = T.edge_census(sim, T.E.STRIDE_CENSUS + ((257, 241, 137),))
sim.close()
print("JSON " + json.dumps({"wrong": wrong, "digest": digest}))
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
    # the default library, here
    import test_gpu_pack_edges as T
    from mptrac_amd import hip
    assert "reference rounding" not in hip.load().mphip_version().decode()
    sim = T.bare_context()
    try:
        wrong, digest = T.edge_census(sim, T.E.STRIDE_CENSUS + ((257, 241, 137),))
    finally:
        sim.close()
    assert wrong == [] and digest == row["digest"]
