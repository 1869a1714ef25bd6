"""HIP_MET_PREP through the drop-in boundary: `trac` and `met_conv` on netCDF files "as stored", with the derived fields
of the reference's meteo preprocessing coming from the device (mphip_derive_met).

Three hourly netCDF files of the seeded atmosphere of tests/refmetprep.py on the "tiny" grid (36 longitudes and the
periodic column, 19 latitudes, 20 levels), written by met_conv from binary files; 3000 particles, two hours, convection
(CONV_CAPE 0), wet and dry deposition, turbulent diffusion with TURB_DX_PBL != TURB_DX_TROP, and module_meteo quantities
that only exist with the preprocessing."""
import os
import struct
import subprocess

import numpy as np
import pytest

import hostfiles as hf
import refmetprep as R
from mptrac_amd import build
from mptrac_amd.synth import Met, synthetic_particles

pytestmark = pytest.mark.gpu

T0 = 707443200.0      # 2022-06-02 00:00 UTC
HOURS = 2
QUANT = ("m", "zg", "pbl", "cape", "pel", "pct", "cl", "o3c")
STORED_3D = ("t", "u", "v", "h2o", "o3", "lwc", "rwc", "iwc", "swc")
STORED_2D = ("ps", "zs", "ts", "us", "vs")
DERIVED_2D = ("o3c", "pbl", "pct", "pcb", "cl", "plcl", "plfc", "pel", "cape", "cin")


def _run(cmd, **kw):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, **kw)
    return r.returncode, r.stdout.decode()


def read_met_bin(path):
    raw = open(path, "rb").read()
    typ, version, time = struct.unpack_from("<iid", raw, 0)
    nx, ny, n = struct.unpack_from("<iii", raw, 16)
    assert (typ, version) == (1, 104)
    off = 28
    axes = []
    for m in (nx, ny, n):
        axes.append(np.frombuffer(raw, dtype=np.float64, count=m, offset=off).copy())
        off += 8 * m
    f2, f3 = {}, {}
    for k in hf.SURF_ORDER:
        f2[k] = np.frombuffer(raw, dtype=np.float32, count=nx * ny, offset=off).reshape(nx, ny).copy()
        off += 4 * nx * ny
    for k in hf.LEVEL_ORDER:
        f3[k] = np.frombuffer(raw, dtype=np.float32, count=nx * ny * n, offset=off).reshape(nx, ny, n).copy()
        off += 4 * nx * ny * n
    assert struct.unpack_from("<i", raw, off)[0] == 999
    return time, axes, f2, f3


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The directory with the netCDF files, the particles and the control file (MET_TYPE 0, HIP_MET_PREP unset)."""
    tmp = str(tmp_path_factory.mktemp("metprep"))
    lib, trac = build.build_host()
    keys = {"NQ": len(QUANT), "METBASE": os.path.join(tmp, "met"), "MET_TYPE": 0, "DT_MET": 3600, "DT_MOD": 180, "ADVECT": 4,
            "DIFFUSION": 1, "TURB_DX_PBL": 60, "TURB_DX_TROP": 40, "CONV_CAPE": 0, "WET_DEPO_IC_A": 1e-3, "WET_DEPO_IC_B": 0.8,
            "WET_DEPO_BC_A": 2e-4, "WET_DEPO_BC_B": 0.8, "DRY_DEPO_VDEP": 0.005, "T_STOP": T0 + 3600.0 * HOURS,
            "ATM_TYPE": 1, "ATM_TYPE_OUT": 1, "ATM_BASENAME": "atm", "ATM_DT_OUT": 3600}
    keys.update({"QNT_NAME[%d]" % i: q for i, q in enumerate(QUANT)})
    hf.write_ctl(os.path.join(tmp, "trac.ctl"), keys)
    open(os.path.join(tmp, "dirlist"), "w").write(tmp + "\n")
    for k in range(HOURS + 1):
        met = R.atmosphere(37, 19, 20, 2024 + k, False, T0 + 3600.0 * k)
        src = hf.met_filename(os.path.join(tmp, "src"), met.time)
        hf.write_met_bin(src, met)
        dst = hf.met_filename(os.path.join(tmp, "met"), met.time)[:-4] + ".nc"
        rc, out = _run([build.MET_CONV_BIN, os.path.join(tmp, "trac.ctl"), src, "1", dst, "0"])
        assert rc == 0, out[-2000:]
    # most particles below 6 km, where the convective columns and the clouds are
    atm = synthetic_particles(3000, time=T0, quantities=QUANT, lon=(-175.0, 175.0), lat=(-75.0, 75.0), z=(0.3, 9.0))
    hf.write_atm_bin(os.path.join(tmp, "atm_in"), atm)
    return dict(tmp=tmp, trac=trac, atm=atm)


def _trac(world, sub, *args):
    """Run trac in a copy of the world's control file under `sub`; returns (exit status, output, directory)."""
    d = os.path.join(world["tmp"], sub)
    os.makedirs(d)
    for name in ("trac.ctl", "atm_in"):
        with open(os.path.join(world["tmp"], name), "rb") as src, open(os.path.join(d, name), "wb") as dst:
            dst.write(src.read())
    open(os.path.join(d, "dirlist"), "w").write(d + "\n")
    rc, out = _run([world["trac"], os.path.join(d, "dirlist"), "trac.ctl", "atm_in", *args])
    return rc, out, d


def _atm_files(d):
    return [os.path.join(d, "atm_2022_06_02_%02d_00_00.bin" % h) for h in range(HOURS + 1)]


@pytest.fixture(scope="module")
def prep_run(world):
    rc, out, d = _trac(world, "prep", "HIP_MET_PREP", "1")
    assert rc == 0, out[-3000:]
    return d


def test_without_the_key_the_run_is_refused_and_the_message_names_it(world):
    rc, out, _ = _trac(world, "refused")
    assert rc != 0 and "HIP_MET_PREP" in out, out[-2000:]


def test_the_run_convects_and_deposits(world, prep_run):
    """Exit status 0, and the modules that need the derived fields really ran.  Nothing but convection moves a particle
    vertically below the tropopause here (no vertical wind in the files, no vertical diffusion there): a changed pressure
    is a convective redistribution.  Above 560 hPa a particle is outside the surface layer of the dry deposition
    everywhere (ps >= 600 hPa, DRY_DEPO_DP 30 hPa): mass lost there at constant pressure went to wet deposition."""
    first, last = (hf.read_atm_bin(f, len(QUANT)) for f in (_atm_files(prep_run)[0], _atm_files(prep_run)[-1]))
    low = first["p"] > 500.
    moved = np.abs(last["p"] - first["p"]) > 1.
    assert (moved & low).any() and (~moved & low).any()
    m0, m1 = first["q"][0], last["q"][0]
    assert (m1 <= m0).all()
    assert ((m1 < m0) & ~moved & (first["p"] < 560.)).any()
    iq = {q: i for i, q in enumerate(QUANT)}
    assert np.isfinite(last["q"][iq["zg"]]).all() and (last["q"][iq["o3c"]] > 100.).all()
    assert (last["q"][iq["pbl"]] > 300.).all() and (np.nan_to_num(last["q"][iq["cape"]]) > 0).any()


def test_met_conv_writes_the_planes_derive_met_returns_and_trac_reads_them(world, prep_run):
    from test_gpu_metprep import bare_context, with_clim
    tmp = world["tmp"]
    sim = with_clim(bare_context())
    try:
        for k in range(HOURS + 1):
            src = hf.met_filename(os.path.join(tmp, "met"), T0 + 3600.0 * k)[:-4] + ".nc"
            dst = hf.met_filename(os.path.join(tmp, "conv"), T0 + 3600.0 * k)
            rc, out = _run([build.MET_CONV_BIN, os.path.join(tmp, "trac.ctl"), src, "0", dst, "1", "HIP_MET_PREP", "1"])
            assert rc == 0, out[-2000:]
            time, (lon, lat, p), f2, f3 = read_met_bin(dst)
            assert time == T0 + 3600.0 * k
            met = Met(time, lon, lat, p, {n: f3[n] for n in STORED_3D}, {n: f2[n] for n in STORED_2D})
            got = sim.derive_met(met, ("geopot", "o3c", "pbl", "cloud", "cape"))
            assert np.array_equal(got["z"], f3["z"]), k
            for name in DERIVED_2D:
                assert np.array_equal(got[name].view(np.uint32), f2[name].view(np.uint32)), (k, name)
            assert np.isfinite(f2["pel"]).any() and np.isnan(f2["pel"]).any()
    finally:
        sim.close()
    rc, out, d = _trac(world, "from_bin", "MET_TYPE", "1", "METBASE", os.path.join(tmp, "conv"))
    assert rc == 0, out[-3000:]
    for a, b in zip(_atm_files(prep_run), _atm_files(d)):
        assert open(a, "rb").read() == open(b, "rb").read(), os.path.basename(a)


def test_read_ahead_thread_derives_the_same(world, prep_run):
    rc, out, d = _trac(world, "prefetch", "HIP_MET_PREP", "1", "HIP_MET_PREFETCH", "1")
    assert rc == 0, out[-3000:]
    assert "Meteo data from the read-ahead" in out
    for a, b in zip(_atm_files(prep_run), _atm_files(d)):
        assert open(a, "rb").read() == open(b, "rb").read(), os.path.basename(a)
