"""HIP_MET_INGEST through the drop-in boundary: `met_conv` from netCDF to MET_TYPE 1 and `trac` give the same bytes with the
reader's own loops (0) and with mphip_ingest_met (1).

The files: one of the reference's coord_test files (Cartesian grid, floats with a fill value below the ground); a global
2 degree longitude / latitude file with both poles written here (so the polar winds and the periodic column both act) as
packed shorts whose fill value is hit below the ground, also with HIP_MET_PREP 2 and MET_DX 2 behind it; the model-level
files of tests/test_gpu_regrid_driver.py (MET_VERT_COORD 1: DECODE, ML2PL, then the other stages in met order).  No file
has a top level that is not finite (there the host loop reads beyond np; include/mptrac_hip.h, at mphip_ingest_met)."""
import os
import subprocess

import numpy as np
import pytest

import hostfiles as hf
from mptrac_amd import build
from mptrac_amd.synth import synthetic_particles
from test_gpu_regrid_driver import MET_P, nc_name, write_model_level_file

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
T0 = 707443200.0      # 2022-06-02 00:00 UTC
HOURS = 2
NX, NY, NP = 180, 91, 20
FILL = -32767


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=180)
    return r.returncode, r.stdout.decode()


def packed(a, lo, hi):
    """int16 codes of `a` over [lo, hi] and their scale_factor / add_offset (as the floats the reader will use)."""
    scale, offset = np.float32((hi - lo) / 64000.0), np.float32(0.5 * (hi + lo))
    q = np.clip(np.round((a - float(offset)) / float(scale)), -32000, 32000).astype(np.int16)
    return q, float(scale), float(offset)


def write_global_file(path, k):
    """Hour k of a global 2 degree snapshot, [lev][lat][lon], packed shorts; below a wavy ground the level fields hold the
    fill value (never on the top levels)."""
    from scipy.io import netcdf_file
    rng = np.random.default_rng(500 + k)
    lon, lat = -180.0 + 2.0 * np.arange(NX), 90.0 - 2.0 * np.arange(NY)
    p = 1000.0 * np.exp(-np.arange(NP) * (7.0 / (NP - 1)))
    lam, phi = np.deg2rad(lon)[None, None, :], np.deg2rad(lat)[None, :, None]
    lev = np.arange(NP)[:, None, None]
    shape = (NP, NY, NX)
    ps = 1000.0 - 250.0 * np.exp(-((lon[None, :] - 80.0) ** 2 + (lat[:, None] - 30.0) ** 2) / 800.0) + 5.0 * np.sin(2 * lam[0] + 0.2 * k)
    below = p[:, None, None] > ps[None, :, :] + 20.0
    assert below.any() and not below[NP // 2:].any()
    fields = dict(t=(285.0 - 3.2 * lev + 10.0 * np.cos(phi) + rng.standard_normal(shape), 150.0, 330.0),
                  u=((20.0 + 2.0 * k) * np.cos(phi) * (1 + 0.05 * lev) + 2.0 * rng.standard_normal(shape), -120.0, 120.0),
                  v=(6.0 * np.sin(2 * lam) * np.cos(phi) + 0.0 * lev + 2.0 * rng.standard_normal(shape), -120.0, 120.0),
                  w=(0.3 * np.sin(lam + phi) * np.sin(np.pi * lev / (NP - 1)) + 0.0 * rng.standard_normal(shape), -3.0, 3.0),
                  q=(8e-3 * np.exp(-lev / 3.0) * (1 + 0.3 * np.cos(phi) * np.sin(lam)) + 0.0 * lev, 0.0, 2e-2),
                  o3=(1e-7 + 8e-6 * np.exp(-((lev - 15.0) / 3.0) ** 2) + 0.0 * lam * phi, 0.0, 2e-5))
    surface = dict(sp=(100.0 * ps, 40000.0, 110000.0), z=(9.80665 * 8.0 * (1000.0 - ps), -500.0, 60000.0),
                   t2m=(288.0 + 10.0 * np.cos(phi[0]) + 0.0 * lam[0], 200.0, 330.0))
    with netcdf_file(path, "w", version=1) as nc:
        nc.createDimension("lon", NX)
        nc.createDimension("lat", NY)
        nc.createDimension("lev", NP)
        nc.createVariable("lon", "d", ("lon",))[:] = lon
        nc.createVariable("lat", "d", ("lat",))[:] = lat
        nc.createVariable("lev", "d", ("lev",))[:] = 100.0 * p
        for name, (a, lo, hi) in list(fields.items()) + list(surface.items()):
            q, scale, offset = packed(np.broadcast_to(a, shape if name in fields else (NY, NX)), lo, hi)
            if name in fields:
                q[below] = FILL
            v = nc.createVariable(name, "h", ("lev", "lat", "lon") if name in fields else ("lat", "lon"))
            v[:] = q
            v.scale_factor, v.add_offset, v._FillValue = np.float64(scale), np.float64(offset), np.int16(FILL)


def conv_both(tmp, src, keys, expect=()):
    """met_conv of `src` to MET_TYPE 1 with HIP_MET_INGEST 0 and 1: the bytes of the two files, and the second log."""
    build.build_host()
    got = []
    for ingest in (0, 1):
        dst = os.path.join(tmp, "out%d_2000_01_01_00.bin" % ingest)
        rc, out = _run([build.MET_CONV_BIN, "-", src, "0", dst, "1", *[str(k) for k in keys], "HIP_MET_INGEST", str(ingest)])
        assert rc == 0, out[-3000:]
        assert ("Ingested on the device" in out) == bool(ingest), out[-3000:]
        got.append(open(dst, "rb").read())
    for text in expect:
        assert text in out, out[-3000:]
    return got


def test_met_conv_of_a_cartesian_float_file_with_fill_values(tmp_path):
    src = os.path.join(HERE, "golden", "ref_coord_test", "era5_utm32_2025_05_01_00.nc")
    keys = ["MET_COORD_TYPE", 1, "MET_UTM_REF_LON", 11.5692782, "MET_UTM_REF_LAT", 48.1507476, "MET_CAPE", 0]
    a, b = conv_both(str(tmp_path), src, keys, expect=("Ingested on the device: decoding extrapolation",))
    assert len(a) > 1000 and a == b


@pytest.fixture(scope="module")
def global_files(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("ingest_global"))
    for k in range(HOURS + 1):
        write_global_file(nc_name(os.path.join(tmp, "met"), T0 + 3600.0 * k), k)
    return tmp


def test_met_conv_of_a_global_packed_file_with_both_poles(global_files, tmp_path):
    src = nc_name(os.path.join(global_files, "met"), T0)
    a, b = conv_both(str(tmp_path), src, [], expect=("Ingested on the device: decoding extrapolation polar winds periodic column",))
    assert len(a) > 4 * (NX + 1) * NY * NP * 5 and a == b


def test_met_conv_of_the_same_file_with_the_preprocessing_and_sampling_behind_it(global_files, tmp_path):
    src = nc_name(os.path.join(global_files, "met"), T0)
    a, b = conv_both(str(tmp_path), src, ["HIP_MET_PREP", 2, "MET_DX", 2], expect=("Sampled on the device: 91 x 91 x 20",))
    assert a == b


@pytest.mark.parametrize("advect_vert_coord", [0, 2])
def test_met_conv_of_a_model_level_file(tmp_path, advect_vert_coord):
    tmp = str(tmp_path)
    src = nc_name(os.path.join(tmp, "ml"), T0)
    write_model_level_file(src, 0)
    keys = ["HIP_MET_PREP", 1, "MET_VERT_COORD", 1, "MET_NP", len(MET_P), "ADVECT_VERT_COORD", advect_vert_coord]
    for i, p in enumerate(MET_P):
        keys += ["MET_P[%d]" % i, p]
    a, b = conv_both(tmp, src, keys, expect=("Ingested on the device: decoding\n", "Interpolated on the device: 12 model levels",
                                             "Ingested on the device: extrapolation polar winds periodic column"))
    assert a == b


def test_trac_with_the_read_ahead_writes_the_same_particle_files(global_files):
    tmp = global_files
    _, trac = build.build_host()
    keys = {"NQ": 1, "QNT_NAME[0]": "m", "METBASE": os.path.join(tmp, "met"), "MET_TYPE": 0, "DT_MET": 3600, "DT_MOD": 180,
            "ADVECT": 4, "MET_DT_OUT": 0, "T_STOP": T0 + 3600.0 * HOURS, "ATM_TYPE": 1, "ATM_TYPE_OUT": 1, "ATM_BASENAME": "atm",
            "ATM_DT_OUT": 3600}
    hf.write_ctl(os.path.join(tmp, "trac.ctl"), keys)
    atm = synthetic_particles(2000, time=T0, quantities=("m",), lon=(-170.0, 170.0), lat=(-85.0, 85.0), z=(1.0, 25.0))
    hf.write_atm_bin(os.path.join(tmp, "atm_in"), atm)
    files = {}
    for sub, args in (("host", ["HIP_MET_INGEST", "0"]), ("device", ["HIP_MET_PREFETCH", "1", "HIP_MET_INGEST", "1"])):
        d = os.path.join(tmp, sub)
        os.makedirs(d)
        for name in ("trac.ctl", "atm_in"):
            with open(os.path.join(tmp, name), "rb") as src, open(os.path.join(d, name), "wb") as dst:
                dst.write(src.read())
        open(os.path.join(d, "dirlist"), "w").write(d + "\n")
        rc, out = _run([trac, os.path.join(d, "dirlist"), "trac.ctl", "atm_in", *args])
        assert rc == 0, out[-3000:]
        if sub == "device":
            assert "Meteo data from the read-ahead" in out and out.count("Ingested on the device") >= HOURS + 1, out[-3000:]
        files[sub] = [open(os.path.join(d, "atm_2022_06_02_%02d_00_00.bin" % h), "rb").read() for h in range(HOURS + 1)]
    assert files["host"] == files["device"] and files["host"][0] != files["host"][-1]


def test_hip_met_ingest_2_is_refused_with_its_message(global_files, tmp_path):
    src = nc_name(os.path.join(global_files, "met"), T0)
    rc, out = _run([build.MET_CONV_BIN, "-", src, "0", str(tmp_path / "out.bin"), "1", "HIP_MET_INGEST", "2"])
    assert rc != 0 and "Set HIP_MET_INGEST to 0 or 1!" in out, out[-2000:]
