"""The edge inputs of the sample and station outputs (tests/analysis_cases.py) in the reference-rounding build
(lib/libmptrac_hip_exact.so), through the functions of tests/test_gpu_analysis_edges.py: the same comparisons, array_equal
everywhere -- the two calls return the host loop's bits in either build.  A process loads one of the two libraries, so
the comparison runs in a child with MPTRAC_AMD_EXACT=1."""
import json
import os
import subprocess
import sys

import pytest

import analysis_cases as AC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
sys.path[:0] = [ROOT, ROOT + "/tests"]
from mptrac_amd import hip
import analysis_cases as AC
import test_gpu_analysis_edges as T
print("library:", hip.load().mphip_version().decode())
for variant in AC.VARIANTS:
    T.sample_decisions(variant)
    T.observation_tiles(variant)
    T.station_decisions(variant)
    T.station_flags(variant)
    for n in AC.COUNTS:
        T.particle_counts(n, variant)
T.not_finite()
T.box_sums_with_the_weighting_functions()
""".replace("ROOT", repr(ROOT))


def test_reference_rounding_build_has_the_host_loops_bits():
    env = dict(os.environ, MPTRAC_AMD_EXACT="1")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert "reference rounding" in lib, lib
    rows = [json.loads(ln[9:]) for ln in res.stdout.splitlines() if ln.startswith("ANA_EDGE ")]
    by = {}
    for r in rows:
        by.setdefault(r["test"], []).append(r)
    nv, ncalls = len(AC.VARIANTS), len(AC.sample_calls())
    # per variant: every sample call of the main case once, `main` again after the long calls, two calls per particle
    # count; the not-finite particles once
    assert len(by["sample"]) == nv * (ncalls + 1 + 2 * len(AC.COUNTS)) + 2
    assert len(by["station"]) == nv * (len(AC.station_calls()) + 3 + len(AC.COUNTS)) + 4
    assert len(by["box_sums"]) == len(AC.kernels())
    assert all(r["differing"] == 0 for r in by["sample"])
    assert all(r["equal"] for r in by["station"] + by["restored"] + by["flags_set"] + by["box_sums"])
    assert all(r["nhit"] == r["reference"] for r in by["cap"]) and all(r["nhit"] == 0 for r in by["listed_once"])
    assert sum(r["records"] for r in by["sample"]) > 10000 and any(r["nan"] for r in by["sample"])
