"""HIP_DEVICE_INTPOL through the drop-in driver: `trac`, one hour, 4000 particles, with the gridded output (MOLMASS and a mass
quantity: the implicit volume mixing ratio reads the temperature at the cell centres), the profile output (t, h2o, o3 at the
box centres) and the sample output (t at the observations) on the observation table of
tests/test_gpu_trac_analysis_device.py.  With the key at 1 the three writers take their meteo values from one
mphip_intpol_met call per output; with 0 from the host interpolation.  On MET_TYPE 1 files and on MET_TYPE 2 files with
HIP_MET_PACKED 1 the grid, profile and sample files are byte for byte the same with both values; on packed files the
driver's summary reports no decode and no host point with 1, and at least one decode with 0."""
import os
import re
import subprocess

import numpy as np
import pytest

import hostfiles as hf
import packfiles as pf
from mptrac_amd.synth import synthetic_met, synthetic_particles
from test_gpu_trac_analysis_device import ANALYSIS, QUANT
from test_host_driver import T0, _setup

pytestmark = pytest.mark.gpu
FILES = ("grid_2022_06_02_00_00_00.tab", "grid_2022_06_02_01_00_00.tab", "prof.tab", "sample.tab")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("intpol"))
    keys = {"NQ": len(QUANT), "GRID_NZ": 3, "GRID_Z0": 0, "GRID_Z1": 30, "SAMPLE_DZ": 5}
    keys.update({"QNT_NAME[%d]" % i: q for i, q in enumerate(QUANT)})
    keys.update({k: v for k, v in ANALYSIS.items() if k.startswith(("SAMPLE", "PROF", "MOLMASS"))})
    trac, mets, _ = _setup(tmp, n=4000, hours=1, extra=keys)
    for k, m in enumerate(mets):          # the files carry ozone: the profile output prints it
        m.f3["o3"] = synthetic_met("tiny", m.time, 1.0 + 0.1 * k, fields=("o3",)).f3["o3"]
        hf.write_met_bin(hf.met_filename(os.path.join(tmp, "met"), m.time), m)
        pf.write_met_pck(pf.met_pck_filename(os.path.join(tmp, "pck"), m.time), m)
    atm = synthetic_particles(4000, time=T0, quantities=QUANT)
    atm["q"][3][:] = 0.0
    atm["q"][4][:] = 0.0
    hf.write_atm_bin(os.path.join(tmp, "atm_in"), atm)
    rows = ["%.2f 5 %d %d %g" % (T0 + 180.0 * (k % 21), lon, lat, float(lon > 0))
            for k, lon in enumerate(range(-175, 180, 10)) for lat in range(-85, 90, 10)]
    rows.sort(key=lambda ln: float(ln.split()[0]))
    open(os.path.join(tmp, "obs.tab"), "w").write("\n".join(rows) + "\n")
    return dict(tmp=tmp, trac=trac)


_runs = {}


def run(world, met_type, intpol, analysis=1):
    key = (met_type, intpol, analysis)
    if key in _runs:
        return _runs[key]
    d = os.path.join(world["tmp"], "run_%d_%d_%d" % key)
    os.makedirs(d)
    for name in ("trac.ctl", "atm_in", "obs.tab"):
        with open(os.path.join(world["tmp"], name), "rb") as a, open(os.path.join(d, name), "wb") as b:
            b.write(a.read())
    open(os.path.join(d, "dirlist"), "w").write(d + "\n")
    args = ["METBASE", os.path.join(world["tmp"], "met" if met_type == 1 else "pck"), "MET_TYPE", str(met_type),
            "HIP_DEVICE_INTPOL", str(intpol), "HIP_DEVICE_ANALYSIS", str(analysis)]
    if met_type == 2:
        args += ["HIP_MET_PACKED", "1"]
    r = subprocess.run([world["trac"], os.path.join(d, "dirlist"), "trac.ctl", "atm_in", *args], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, cwd=d, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    decodes = re.search(r"MET_DECODES = (\d+)", out)
    points = re.search(r"INTPOL_POINTS = (\d+) host, (\d+) device", out)
    assert decodes and points and "PARTICLE_DOWNLOADS" in out, out[-2000:]
    files = {f: open(os.path.join(d, f), "rb").read() for f in FILES}
    assert all(len(v) > 0 for v in files.values())
    _runs[key] = dict(dir=d, files=files, decodes=int(decodes.group(1)), host=int(points.group(1)), device=int(points.group(2)))
    return _runs[key]


@pytest.mark.parametrize("met_type", [1, 2])
def test_the_files_are_the_same_bytes_with_both_values_of_the_key(world, met_type):
    host, device = run(world, met_type, 0), run(world, met_type, 1)
    for f in FILES:
        assert host["files"][f] == device["files"][f], f
    assert host["device"] == 0 and host["host"] > 0
    assert device["host"] == 0 and device["device"] == host["host"]       # the same points, and only those
    # the files hold what the test is about: implicit mixing ratios, profile rows with ozone, sample rows with a mixing ratio
    grid = np.loadtxt(os.path.join(device["dir"], FILES[1]), ndmin=2)
    assert np.count_nonzero(grid[:, 7] > 0) > 100
    prof = np.loadtxt(os.path.join(device["dir"], "prof.tab"), ndmin=2)
    assert len(prof) > 100 and (prof[:, 5] > 150).all() and (prof[:, 8] > 0).all() and (prof[:, 7] > 0).any()
    sample = np.loadtxt(os.path.join(device["dir"], "sample.tab"), ndmin=2)
    assert np.count_nonzero(sample[:, 8] > 0) > 50


def test_packed_snapshots_stay_codes_with_the_key(world):
    host, device = run(world, 2, 0), run(world, 2, 1)
    assert device["decodes"] == 0 and device["host"] == 0 and device["device"] > 0
    assert host["decodes"] >= 1
    # (and the packed meteorology is not the float one: the two file types give other bytes)
    assert run(world, 1, 1)["files"]["prof.tab"] != device["files"]["prof.tab"]


def test_host_particle_loops_with_device_meteo_values(world):
    """HIP_DEVICE_ANALYSIS 0 (the writers loop over downloaded particles) together with HIP_DEVICE_INTPOL 1"""
    both, mixed = run(world, 2, 1), run(world, 2, 1, analysis=0)
    for f in FILES:
        assert both["files"][f] == mixed["files"][f], f
    assert mixed["decodes"] == 0 and mixed["host"] == 0 and mixed["device"] == both["device"]
