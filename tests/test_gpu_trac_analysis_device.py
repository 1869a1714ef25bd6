"""The drop-in driver with the CSI, profile, sample and station outputs in every time step: HIP_DEVICE_ANALYSIS 1 (the
default: their particle loops run on the device, the particles are downloaded only for particle / ensemble / VTK files)
against HIP_DEVICE_ANALYSIS 0 (a download per step and the host loops).  The files are byte for byte the same, the `stat`
flags of the final particle file included, and the driver's summary reports the downloads."""
import filecmp
import os
import re
import subprocess

import numpy as np
import pytest

import hostfiles as hf
from mptrac_amd.synth import synthetic_particles
from test_host_driver import T0, _setup

pytestmark = pytest.mark.gpu

QUANT = ("m", "rp", "rhop", "stat", "ens")
ANALYSIS = {"STAT_BASENAME": "station", "STAT_LON": 10, "STAT_LAT": 20, "STAT_R": 1500, "CSI_BASENAME": "csi",
            "CSI_DT_OUT": 3600, "CSI_OBSFILE": "obs.tab", "CSI_NX": 36, "CSI_NY": 18, "CSI_MODMIN": 1e-12, "CSI_OBSMIN": 0.5,
            "SAMPLE_BASENAME": "sample", "SAMPLE_OBSFILE": "obs.tab", "SAMPLE_DX": 800, "PROF_BASENAME": "prof",
            "PROF_OBSFILE": "obs.tab", "PROF_NX": 36, "PROF_NY": 18, "PROF_NZ": 10, "MOLMASS": 64}


def _particles(placed=None):
    atm = synthetic_particles(4000, time=T0, quantities=QUANT)
    atm["q"][3][:] = 0.0
    atm["q"][4][:] = np.arange(4000) % 4
    for name, values in (placed[0] if placed else {}).items():
        (atm["q"][0] if name == "m" else atm[name])[:len(values)] = values
    return atm


def _run(tmp, extra, key, placed=None):
    """`placed`: (particle columns {name: values} that replace the first particles, observation lines of the first step,
    files {name: text}) -- see test_device_analysis_with_300_observations_in_one_time_step"""
    os.makedirs(tmp)
    keys = {"NQ": len(QUANT), "GRID_STDDEV": 1, "GRID_NZ": 3, "GRID_Z0": 0, "GRID_Z1": 30, "HIP_LOCALITY_SORT_INTERVAL": 3,
            "HIP_DEVICE_ANALYSIS": key}
    keys.update({"QNT_NAME[%d]" % i: q for i, q in enumerate(QUANT)})
    keys.update(extra)
    trac, _, _ = _setup(tmp, n=4000, hours=1, extra=keys)
    atm = _particles(placed)
    hf.write_atm_bin(os.path.join(tmp, "atm_in"), atm)
    lines = list(placed[1]) if placed else []
    for k, lon in enumerate(range(-175, 180, 10)):      # observations in every step of the hour
        for lat in range(-85, 90, 10):
            if not (placed and k % 21 == 0):
                lines.append("%.2f 5 %d %d %g" % (T0 + 180.0 * (k % 21), lon, lat, float(lon > 0)))
    lines = sorted(lines, key=lambda ln: float(ln.split()[0]))
    open(os.path.join(tmp, "obs.tab"), "w").write("\n".join(lines) + "\n")
    for name, text in (placed[2] if placed else {}).items():
        open(os.path.join(tmp, name), "w").write(text)
    r = subprocess.run([trac, os.path.join(tmp, "dirlist"), "trac.ctl", "atm_in"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, cwd=tmp)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    m = re.search(r"PARTICLE_DOWNLOADS = (\d+)\s+\(by mptrac_write_output in (\d+) calls", out)
    assert m, out[-2000:]
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("setup", ["all four outputs", "CSI and samples only, no particle file before T_STOP"])
def test_device_analysis_writes_the_files_of_the_host_loops(tmp_path, setup):
    if setup == "all four outputs":
        extra, files, due = dict(ANALYSIS), ["csi.tab", "prof.tab", "sample.tab", "station.tab"], 2     # particle files at T0 and T_STOP
    else:
        extra = {k: v for k, v in ANALYSIS.items() if k.startswith(("CSI", "SAMPLE"))}
        extra.update({"ATM_DT_OUT": 86400 * 365, "GRID_BASENAME": "-"})
        files, due = ["csi.tab", "sample.tab"], 1                                                      # ... at T_STOP only
    host, device = str(tmp_path / "host"), str(tmp_path / "device")
    downloads0, calls0 = _run(host, extra, 0)
    downloads1, calls1 = _run(device, extra, 1)
    assert calls0 == calls1 == 21
    assert downloads0 == calls0           # the host loops: a download in every time step
    assert downloads1 <= due              # the device loops: only where a particle file is due
    for name in files + ["atm_2022_06_02_01_00_00.bin"]:
        assert os.path.getsize(os.path.join(host, name)) > 0, name
        assert filecmp.cmp(os.path.join(host, name), os.path.join(device, name), shallow=False), name
    sample = np.loadtxt(os.path.join(device, "sample.tab"), ndmin=2)
    assert len(sample) > 300 and np.count_nonzero(sample[:, 6]) > 100      # observations in many steps, particles around them
    if "station.tab" in files:
        rows = np.loadtxt(os.path.join(device, "station.tab"), ndmin=2)
        flags = hf.read_atm_bin(os.path.join(device, "atm_2022_06_02_01_00_00.bin"), len(QUANT))["q"][3]
        assert len(rows) > 20 and int(flags.sum()) == len(rows)


def test_device_analysis_with_300_observations_in_one_time_step(tmp_path):
    """The multi-tile path of the sample output through the driver: 300 observations in the first time step (more than
    one LDS tile of 256), the clusters of tests/analysis_cases.py around some of them -- crowded observations at the
    indices 0, 255, 256 and 299, two identical ones, masses over 16 decades -- a layer depth and a weighting
    function; the station sits at a cluster's particle.  HIP_DEVICE_ANALYSIS 0 and 1 write the same bytes, and the counts
    of the first step are those of tests/refanalysis.py on the particle file: the reference of the edge tests and
    output.c agree on this path too."""
    import analysis_cases as AC
    import refanalysis as RA
    obs, rows = AC.clusters(np.random.default_rng(20260))
    by = {o[0]: o for o in obs}
    layout = AC.tiled(300)
    layout = [by.get(o[0], o) for o in layout]
    assert [layout[i][0] for i in (0, 255, 256, 299)] == ["list/65", "list/129", "list/128", "list/65b"]
    columns = {"lon": [r[0] for r in rows], "lat": [r[1] for r in rows], "p": [r[2] for r in rows], "m": [r[4] for r in rows]}
    at = next(r for r in rows if r[6].startswith("cluster/129/"))      # the station: at a particle of the largest cluster
    kz, kw = AC.kernels()["nk5"]
    files = {"kernel.tab": "".join("%.17g %.17g\n" % zw for zw in zip(kz, kw))}
    lines = ["%.2f %.17g %.17g %.17g %d" % (T0, o[3], o[1], o[2], i % 2) for i, o in enumerate(layout)]
    placed = (columns, lines, files)
    extra = {k: v for k, v in ANALYSIS.items() if k.startswith(("SAMPLE", "STAT", "MOLMASS"))}
    extra.update({"SAMPLE_DZ": AC.DZ, "SAMPLE_KERNEL": "kernel.tab", "STAT_LON": at[0], "STAT_LAT": at[1], "STAT_R": 800,
                  "GRID_BASENAME": "-"})
    host, device = str(tmp_path / "host"), str(tmp_path / "device")
    _run(host, extra, 0, placed)
    _run(device, extra, 1, placed)
    for name in ("sample.tab", "station.tab", "atm_2022_06_02_01_00_00.bin"):
        assert os.path.getsize(os.path.join(host, name)) > 0, name
        assert filecmp.cmp(os.path.join(host, name), os.path.join(device, name), shallow=False), name
    atm = _particles(placed)
    lon, lat, z = AC.obs_arrays(layout)
    count, mass, _, _ = RA.sample_obs(atm, T0 - 90.0, T0 + 90.0, lon, lat, z, ANALYSIS["SAMPLE_DX"], AC.DZ, 0, (kz, kw))
    assert count[255] >= 129 and count[256] >= 128 and count[0] == count[299] >= 65 and count.min() < 10
    sample = np.loadtxt(os.path.join(device, "sample.tab"), ndmin=2)
    first = sample[sample[:, 0] == T0]
    assert len(first) == 300 and np.array_equal(first[:, 6].astype(int), count)
    listed = RA.station_hits(atm, T0, 180.0, at[0], at[1], 800.0, -1e100, 1e100, 3)[0]
    station = np.loadtxt(os.path.join(device, "station.tab"), ndmin=2)
    assert len(listed) >= 100 and np.count_nonzero(station[:, 0] == T0) == len(listed)
