"""HIP_DEVICE_SELECT through the drop-in driver: `trac`, one hour, 4000 particles of which every third is released half an
hour after the first output time (so ATM_FILTER 2 and the VTK window drop some), ASCII particle files with ATM_STRIDE 7
and VTK files with VTK_STRIDE 50 every half hour, the locality order in force (HIP_LOCALITY_SORT_INTERVAL 3).  With the key
at 1 both writers take their rows from one mphip_select_atm call; with 0 from downloaded particles.  Every particle and
VTK file is byte for byte the same with both values; with 1 the driver's summary reports no particle download where only
these outputs are due, and as many as with 0 when the ensemble output is due as well."""
import filecmp
import os
import re
import subprocess

import pytest

import hostfiles as hf
from mptrac_amd.synth import synthetic_particles
from test_host_driver import T0, _setup

pytestmark = pytest.mark.gpu
QUANT = ("m", "rp", "rhop", "ens")
STAMPS = ("2022_06_02_00_00_00", "2022_06_02_00_30_00", "2022_06_02_01_00_00")
FILES = tuple("atm_%s.tab" % s for s in STAMPS) + tuple("vtk_%05d.vtk" % k for k in (1, 2, 3))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("select"))
    keys = {"NQ": len(QUANT), "ATM_TYPE_OUT": 0, "ATM_STRIDE": 7, "ATM_DT_OUT": 1800, "VTK_BASENAME": "vtk", "VTK_STRIDE": 50,
            "VTK_DT_OUT": 1800, "HIP_LOCALITY_SORT_INTERVAL": 3, "GRID_BASENAME": "-"}
    keys.update({"QNT_NAME[%d]" % i: q for i, q in enumerate(QUANT)})
    trac, _, _ = _setup(tmp, n=4000, hours=1, extra=keys)
    atm = synthetic_particles(4000, time=T0, quantities=QUANT)
    atm["time"][::3] = T0 + 1800.0          # released after the first output time
    atm["q"][3][:] = 0.0                    # one ensemble member
    hf.write_atm_bin(os.path.join(tmp, "atm_in"), atm)
    return dict(tmp=tmp, trac=trac)


_runs = {}


def run(world, atm_filter, select, ens=False):
    key = (atm_filter, select, ens)
    if key in _runs:
        return _runs[key]
    d = os.path.join(world["tmp"], "run_%d_%d_%d" % key)
    os.makedirs(d)
    for name in ("trac.ctl", "atm_in"):
        with open(os.path.join(world["tmp"], name), "rb") as a, open(os.path.join(d, name), "wb") as b:
            b.write(a.read())
    open(os.path.join(d, "dirlist"), "w").write(d + "\n")
    args = ["ATM_FILTER", str(atm_filter), "HIP_DEVICE_SELECT", str(select)]
    if ens:
        args += ["ENS_BASENAME", "ens", "ENS_DT_OUT", "1800"]
    r = subprocess.run([world["trac"], os.path.join(d, "dirlist"), "trac.ctl", "atm_in", *args], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, cwd=d, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    downloads = re.search(r"PARTICLE_DOWNLOADS = (\d+)", out)
    assert downloads, out[-2000:]
    _runs[key] = dict(dir=d, downloads=int(downloads.group(1)))
    print("SELECT_DRIVER", key, _runs[key]["downloads"])
    return _runs[key]


def rows_of(path):
    return [ln for ln in open(path) if ln.strip() and not ln.startswith("#")]


@pytest.mark.parametrize("atm_filter", [0, 1, 2])
def test_the_files_are_the_same_bytes_without_a_download(world, atm_filter):
    host, device = run(world, atm_filter, 0), run(world, atm_filter, 1)
    for f in FILES:
        a, b = os.path.join(host["dir"], f), os.path.join(device["dir"], f)
        assert os.path.getsize(a) > 0 and os.path.getsize(b) > 0, f
        assert filecmp.cmp(a, b, shallow=False), f
    assert host["downloads"] == 3 and device["downloads"] == 0
    # the files hold what the test is about: every 7th particle; filter 2 drops the particles not yet released from
    # the first file, filter 1 blanks their quantities; the VTK window drops them from the first point cloud
    first, second = (rows_of(os.path.join(device["dir"], FILES[k])) for k in (0, 1))
    assert len(second) == (4000 + 6) // 7
    assert len(first) == (len(second) if atm_filter < 2 else sum(1 for e in range(0, 4000, 7) if e % 3))
    assert any("nan" in ln for ln in first) == (atm_filter == 1)
    points = [int(re.search(r"POINTS (\d+) float", open(os.path.join(device["dir"], FILES[k])).read()).group(1)) for k in (3, 4)]
    assert points == [sum(1 for e in range(0, 4000, 50) if e % 3), 80]


def test_the_filtered_file_is_shorter(world):
    a, b = (os.path.join(run(world, f, 1)["dir"], FILES[0]) for f in (2, 0))
    assert 0 < os.path.getsize(a) < os.path.getsize(b)


def test_an_ensemble_output_keeps_the_downloads(world):
    host, device = run(world, 2, 0, ens=True), run(world, 2, 1, ens=True)
    assert host["downloads"] == device["downloads"] == 3
    for f in FILES + tuple("ens_%s.tab" % s for s in STAMPS):
        assert filecmp.cmp(os.path.join(host["dir"], f), os.path.join(device["dir"], f), shallow=False), f
    assert filecmp.cmp(os.path.join(device["dir"], FILES[0]), os.path.join(run(world, 2, 1)["dir"], FILES[0]), shallow=False)
