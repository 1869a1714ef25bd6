"""The analysis outputs on the device (mphip_box_sums, mphip_sample_obs, mphip_station_hits) and the wide cos / sin they
rest on in the reference-rounding build (lib/libmptrac_hip_exact.so): the comparisons of tests/test_gpu_analysis_outputs.py
-- counts, hit lists, flags and sums array_equal to the transcription of the host loops -- hold there as well.  A process
loads one of the two libraries, so they run in a child with MPTRAC_AMD_EXACT=1, which reports the library it loaded."""
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
import test_gpu_analysis_outputs as T
print("library:", hip.load().mphip_version().decode())
for n in (97, 6000):
    for interval in (0, 3):
        s, t, dt = T._stepped(n, -180.0, interval)
        T._check_everything(s, t, dt, n, -180.0, long_chain=False)
        s.close()
        print("DONE stepped", n, interval, flush=True)
    for steps in (0, 1):
        s, t, dt = T._stepped(n, 0.0, 3, steps=steps)
        T._check_everything(s, t, dt, n, 0.0, long_chain=False)
        s.close()
        print("DONE 0_360", n, steps, flush=True)
T.test_wide_cos_sin_on_the_device_are_the_c_librarys()
print("DONE wide", flush=True)
T.test_error_returns()
print("DONE errors", flush=True)
T.test_two_index_range_shards_give_the_sums_of_the_partials()
print("DONE shards", flush=True)
""".replace("ROOT", repr(ROOT))


def test_reference_rounding_build_equals_the_host_loops_too():
    env = dict(os.environ, MPTRAC_AMD_EXACT="1")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert "reference rounding" in lib, lib
    done = [ln[5:] for ln in res.stdout.splitlines() if ln.startswith("DONE ")]
    want = ["stepped %d %d" % (n, i) for n in (97, 6000) for i in (0, 3)] + ["0_360 %d %d" % (n, k) for n in (97, 6000) for k in (0, 1)]
    assert sorted(done) == sorted(want + ["wide", "errors", "shards"]), done
