"""The regridding of netCDF input through the drop-in boundary: `met_conv` and `trac` on model-level files (MET_VERT_COORD 1,
MET_NP, MET_P) and on pressure-level files that are down-sampled with smoothing (MET_DX ... MET_SP), with HIP_MET_PREP 1
(mphip_regrid_met).

Three hourly model-level files on the "tiny" grid of tests/refmetprep.py (36 longitudes -- the reader adds the periodic
column --, 19 latitudes) with 12 model levels whose 3-D pressure follows a smooth surface pressure, written with
scipy.io.netcdf_file.  The reference-rounding library stands in front of the C tools where bits are compared (the
switch a C user has: same ABI)."""
import os
import subprocess

import numpy as np
import pytest

import cases
import hostfiles as hf
import refmetprep
import refregrid as R
from mptrac_amd import build
from mptrac_amd.clim import load_clim_tropo
from mptrac_amd.ctl import ctl_from_quantities
from mptrac_amd.synth import Met, synthetic_particles
from test_gpu_metprep_driver import read_met_bin

pytestmark = pytest.mark.gpu

T0 = 707443200.0      # 2022-06-02 00:00 UTC
HOURS = 2
NLEV = 12
MET_P = (1000.0, 850.0, 700.0, 500.0, 300.0, 150.0, 50.0, 10.0)      # 1000 hPa lies below many surfaces: clamped
ML_FIELDS = ("t", "u", "v", "w", "h2o")
MA, MH2O = 28.9644, 18.01528


def _run(cmd, exact=False, **kw):
    env = dict(os.environ)
    if exact:      # in front of what is preloaded already, not instead of it
        env["LD_PRELOAD"] = ":".join(x for x in (build.build_hip_exact(), env.get("LD_PRELOAD", "")) if x)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, env=env, **kw)
    return r.returncode, r.stdout.decode()


def nc_name(base, t):
    return hf.met_filename(base, t)[:-4] + ".nc"


def model_level_snapshot(k):
    """What the file of hour k holds (its own units, [lev][lat][lon]) and what the reader makes of it ([lon][lat][lev],
    the units of met_t: the reader multiplies in float)."""
    rng = np.random.default_rng(77 + k)
    lon = -180.0 + 10.0 * np.arange(36)
    lat = np.linspace(-80.0, 80.0, 19)
    lam, phi = np.deg2rad(lon)[:, None], np.deg2rad(lat)[None, :]
    ps = 99000.0 + 2500.0 * np.sin(2 * lam + 0.3 * k) * np.cos(phi) - 6000.0 * np.exp(-((lon[:, None] - 40) ** 2 + lat[None, :] ** 2) / 900.0)
    eta = np.arange(NLEV) / (NLEV - 1)
    pl = 500.0 + (ps[:, :, None] - 500.0) * (1.0 - eta)[None, None, :] ** 2          # Pa, k = 0 at the surface
    rel = pl / ps[:, :, None]
    shape = pl.shape
    f = dict(pl=pl, t=215.0 + 75.0 * rel + 0.5 * rng.standard_normal(shape),
             u=(25.0 + 3.0 * k) * np.cos(phi)[:, :, None] * (1.2 - rel) + rng.standard_normal(shape),
             v=8.0 * np.sin(3 * lam)[:, :, None] * np.ones(shape) + rng.standard_normal(shape),
             w=0.2 * np.sin(2 * lam + phi)[:, :, None] * np.sin(np.pi * rel),
             q=8e-3 * rel ** 3 * (1.0 + 0.1 * rng.standard_normal(shape)))
    file3 = {n: np.ascontiguousarray(a, dtype=np.float32) for n, a in f.items()}
    file2 = dict(sp=ps.astype(np.float32), t2m=(288.0 + rng.standard_normal(ps.shape)).astype(np.float32))
    scale = dict(pl=0.01, t=1.0, u=1.0, v=1.0, w=0.01, q=MA / MH2O)
    met3 = {("h2o" if n == "q" else n): (np.float32(scale[n]) * a).astype(np.float32) for n, a in file3.items()}
    met2 = dict(ps=(np.float32(0.01) * file2["sp"]).astype(np.float32), ts=file2["t2m"])
    return lon, lat, file3, file2, met3, met2


def write_model_level_file(path, k):
    from scipy.io import netcdf_file
    lon, lat, file3, file2, _, _ = model_level_snapshot(k)
    with netcdf_file(path, "w", version=1) as nc:
        nc.createDimension("lon", len(lon))
        nc.createDimension("lat", len(lat))
        nc.createDimension("lev", NLEV)
        nc.createVariable("lon", "d", ("lon",))[:] = lon
        nc.createVariable("lat", "d", ("lat",))[:] = lat
        for n, a in file3.items():
            nc.createVariable(n, "f", ("lev", "lat", "lon"))[:] = a.transpose(2, 1, 0)
        for n, a in file2.items():
            nc.createVariable(n, "f", ("lat", "lon"))[:] = a.transpose(1, 0)


def periodic(a):
    return np.concatenate([a, a[:1]], axis=0)


def expected_snapshot(k):
    """The snapshot the reader holds after ML2PL and the periodic column, by the restatement; with the kept model-level
    fields."""
    lon, lat, _, _, met3, met2 = model_level_snapshot(k)
    snap = R.Snap(lon, lat, np.arange(NLEV), met3, met2, time=T0 + 3600.0 * k)
    pl = R.ml2pl(snap, MET_P)
    f3 = {n: periodic(a) for n, a in pl.f3.items()}
    f3.update(pl=periodic(met3["pl"]), ul=periodic(met3["u"]), vl=periodic(met3["v"]), wl=periodic(met3["w"]))
    f2 = {n: periodic(a) for n, a in met2.items()}
    return np.append(lon, 180.0), lat, f3, f2


@pytest.fixture(scope="module")
def ml_world(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("regrid_ml"))
    _, trac = build.build_host()
    keys = {"NQ": 1, "QNT_NAME[0]": "m", "METBASE": os.path.join(tmp, "met"), "MET_TYPE": 0, "DT_MET": 3600, "DT_MOD": 180,
            "ADVECT": 4, "MET_DT_OUT": 0, "T_STOP": T0 + 3600.0 * HOURS, "ATM_TYPE": 1, "ATM_TYPE_OUT": 1, "ATM_BASENAME": "atm",
            "ATM_DT_OUT": 3600, "HIP_MET_PREP": 1, "MET_VERT_COORD": 1, "MET_NP": len(MET_P)}
    keys.update({"MET_P[%d]" % i: p for i, p in enumerate(MET_P)})
    hf.write_ctl(os.path.join(tmp, "trac.ctl"), keys)
    for k in range(HOURS + 1):
        write_model_level_file(nc_name(os.path.join(tmp, "met"), T0 + 3600.0 * k), k)
    atm = synthetic_particles(2000, time=T0, quantities=("m",), lon=(-170.0, 170.0), lat=(-70.0, 70.0), z=(1.0, 25.0))
    hf.write_atm_bin(os.path.join(tmp, "atm_in"), atm)
    return dict(tmp=tmp, trac=trac, atm=atm)


def _trac(world, sub, *args, exact=False):
    d = os.path.join(world["tmp"], sub)
    os.makedirs(d)
    for name in ("trac.ctl", "atm_in"):
        with open(os.path.join(world["tmp"], name), "rb") as src, open(os.path.join(d, name), "wb") as dst:
            dst.write(src.read())
    open(os.path.join(d, "dirlist"), "w").write(d + "\n")
    rc, out = _run([world["trac"], os.path.join(d, "dirlist"), "trac.ctl", "atm_in", *args], exact=exact)
    return rc, out, d


def _atm_files(d):
    return [os.path.join(d, "atm_2022_06_02_%02d_00_00.bin" % h) for h in range(HOURS + 1)]


def test_met_conv_turns_model_level_files_into_pressure_level_files(ml_world):
    """Under the reference-rounding library the level fields of the binary files are the restatement's bits."""
    tmp = ml_world["tmp"]
    for k in range(HOURS + 1):
        t = T0 + 3600.0 * k
        dst = hf.met_filename(os.path.join(tmp, "conv"), t)
        rc, out = _run([build.MET_CONV_BIN, os.path.join(tmp, "trac.ctl"), nc_name(os.path.join(tmp, "met"), t), "0", dst, "1"],
                       exact=True)
        assert rc == 0 and "reference rounding" in out, out[-2000:]
        time, (lon, lat, p), f2, f3 = read_met_bin(dst)
        want_lon, want_lat, want3, want2 = expected_snapshot(k)
        assert time == t and np.array_equal(lon, want_lon) and np.array_equal(lat, want_lat) and np.array_equal(p, MET_P)
        for n in ML_FIELDS:
            assert np.array_equal(f3[n].view(np.uint32), want3[n].view(np.uint32)), (k, n)
        assert np.array_equal(f2["ps"], want2["ps"]) and np.array_equal(f2["ts"], want2["ts"])


def test_trac_advects_on_the_files_model_levels_like_the_oracle(ml_world):
    """ADVECT_VERT_COORD 2 from model-level netCDF files: exit status 0, and the particles of the oracle stepping the same
    ul, vl, wl, pl and the restatement's pressure-level fields, to the 1e-10 of tests/test_host_driver.py."""
    from oracle import binding as B
    rc, out, d = _trac(ml_world, "mlp", "ADVECT_VERT_COORD", "2")
    assert rc == 0, out[-3000:]
    mets = []
    for k in range(HOURS + 1):
        lon, lat, f3, f2 = expected_snapshot(k)
        zero3 = np.zeros(f3["t"].shape, dtype=np.float32)
        zero2 = np.zeros(f2["ps"].shape, dtype=np.float32)
        for n in cases.PRESSURE_LEVEL_FIELDS:
            if n not in f3 and n not in f2:
                (f3 if n in ("lwc", "rwc", "iwc", "swc") else f2)[n] = zero3 if n in ("lwc", "rwc", "iwc", "swc") else zero2
        f2["pbl"] = f2["ps"] - np.float32(100.0)
        mets.append(Met(T0 + 3600.0 * k, lon, lat, np.array(MET_P), f3, f2))
        assert mets[-1].npl == NLEV and mets[-1].np == len(MET_P)
    ctl = dict(advect=4, advect_vert_coord=2, dt_mod=180.0, dt_met=3600.0, t_stop=T0 + 3600.0 * HOURS, met_dt_out=0.0,
               **ctl_from_quantities(("m",)))
    o = B.Oracle(ctl, load_clim_tropo(), mets[0], mets[1], ml_world["atm"])
    o.timesteps_init()
    imet, snaps = 0, {}
    for t in cases.step_times(o.ctl):
        while t > o.met[1].time:
            imet += 1
            o.swap_met(mets[imet + 1])
        o.run_timestep(t)
        if (t - T0) % 3600.0 == 0:
            snaps[t] = o.state()
    first = hf.read_atm_bin(_atm_files(d)[0], 1)
    for hour, f in enumerate(_atm_files(d)):
        got, ref = hf.read_atm_bin(f, 1), snaps[T0 + 3600.0 * hour] if hour else None
        if hour == 0:
            continue
        assert np.array_equal(got["time"], ref["time"])
        for name in ("lon", "lat", "p"):
            assert cases.rel_err(got[name], ref[name]) <= 1e-10, (hour, name, cases.rel_err(got[name], ref[name]))
        assert cases.rel_err(got["q"], ref["q"]) <= 1e-10
    last = hf.read_atm_bin(_atm_files(d)[-1], 1)
    assert (np.abs(last["p"] - first["p"]) > 0.1).any() and (np.abs(last["lon"] - first["lon"]) > 0.1).any()


def test_model_level_winds_differ_from_pressure_level_winds(ml_world):
    """The same files with ADVECT_VERT_COORD 0 run too, and end elsewhere: the model-level path is really taken above."""
    rc, out, d = _trac(ml_world, "pl")
    assert rc == 0, out[-3000:]
    rc2, out2, d2 = _trac(ml_world, "mlp_again", "ADVECT_VERT_COORD", "2")
    assert rc2 == 0, out2[-3000:]
    a, b = hf.read_atm_bin(_atm_files(d)[-1], 1), hf.read_atm_bin(_atm_files(d2)[-1], 1)
    assert np.isfinite(a["p"]).all() and not np.array_equal(a["lon"], b["lon"])


def test_without_hip_met_prep_model_level_input_is_refused(ml_world):
    rc, out, _ = _trac(ml_world, "refused", "HIP_MET_PREP", "0")
    assert rc != 0 and "HIP_MET_PREP" in out and "MET_VERT_COORD" in out, out[-2000:]


def test_model_level_advection_with_sampling_is_refused(ml_world):
    rc, out, _ = _trac(ml_world, "refused_dx", "ADVECT_VERT_COORD", "2", "MET_DX", "2")
    assert rc != 0 and "MET_DX" in out and "not sampled" in out, out[-2000:]


def test_a_model_level_file_without_its_pressure_stops_with_a_message(ml_world, tmp_path):
    """The pressure-level files of the sampling test below have no 3-D pressure variable."""
    from scipy.io import netcdf_file
    tmp = str(tmp_path)
    src = nc_name(os.path.join(ml_world["tmp"], "met"), T0)
    dst = nc_name(os.path.join(tmp, "nopl"), T0)
    with netcdf_file(src, "r", mmap=False) as a, netcdf_file(dst, "w", version=1) as b:
        for n, size in a.dimensions.items():
            b.createDimension(n, size)
        for n, v in a.variables.items():
            if n != "pl":
                b.createVariable(n, v.data.dtype.char, v.dimensions)[:] = v.data
    rc, out = _run([build.MET_CONV_BIN, os.path.join(ml_world["tmp"], "trac.ctl"), dst, "0", os.path.join(tmp, "out.bin"), "1"])
    assert rc != 0 and "3-D pressure" in out, out[-2000:]


# ---- down-sampling with smoothing ------------------------------------------------------------------------------------------

def test_trac_on_sampled_input_equals_a_run_on_files_sampled_beforehand(tmp_path):
    """MET_DX 2 MET_SX 2 on pressure-level netCDF files against binary files the restatement sampled from what the reader
    holds (the netCDF files converted back by met_conv: the periodic column included); byte for byte under the
    reference-rounding library."""
    tmp = str(tmp_path)
    _, trac = build.build_host()
    keys = {"NQ": 1, "QNT_NAME[0]": "m", "METBASE": os.path.join(tmp, "met"), "MET_TYPE": 0, "DT_MET": 3600, "DT_MOD": 180,
            "ADVECT": 4, "MET_DT_OUT": 0, "T_STOP": T0 + 3600.0 * HOURS, "ATM_TYPE": 1, "ATM_TYPE_OUT": 1, "ATM_BASENAME": "atm",
            "ATM_DT_OUT": 3600}
    hf.write_ctl(os.path.join(tmp, "trac.ctl"), keys)
    ctl = os.path.join(tmp, "trac.ctl")
    for k in range(HOURS + 1):
        t = T0 + 3600.0 * k
        met = refmetprep.atmosphere(37, 19, 20, 2024 + k, False, t)
        src, nc = hf.met_filename(os.path.join(tmp, "src"), t), nc_name(os.path.join(tmp, "met"), t)
        hf.write_met_bin(src, met)
        rc, out = _run([build.MET_CONV_BIN, ctl, src, "1", nc, "0"])
        assert rc == 0, out[-2000:]
        held = hf.met_filename(os.path.join(tmp, "held"), t)
        rc, out = _run([build.MET_CONV_BIN, ctl, nc, "0", held, "1"])
        assert rc == 0, out[-2000:]
        time, (lon, lat, p), f2, f3 = read_met_bin(held)
        assert len(lon) == 37
        pre = R.sample(R.Snap(lon, lat, p, {n: f3[n] for n in R.ML_FIELDS}, f2, time=t), (2, 1, 1), (2, 1, 1))
        assert (pre.nx, pre.ny, pre.np) == (19, 19, 20)
        hf.write_met_bin(hf.met_filename(os.path.join(tmp, "pre"), t), Met(t, pre.lon, pre.lat, pre.p, pre.f3, pre.f2))
    atm = synthetic_particles(2000, time=T0, quantities=("m",), lon=(-170.0, 170.0), lat=(-70.0, 70.0), z=(1.0, 25.0))
    hf.write_atm_bin(os.path.join(tmp, "atm_in"), atm)
    world = dict(tmp=tmp, trac=trac)
    rc, out, a = _trac(world, "on_the_fly", "HIP_MET_PREP", "1", "MET_DX", "2", "MET_SX", "2", exact=True)
    assert rc == 0 and "Sampled on the device: 19 x 19 x 20" in out, out[-3000:]
    rc, out, b = _trac(world, "beforehand", "MET_TYPE", "1", "METBASE", os.path.join(tmp, "pre"), exact=True)
    assert rc == 0, out[-3000:]
    for fa, fb in zip(_atm_files(a), _atm_files(b)):
        assert open(fa, "rb").read() == open(fb, "rb").read(), os.path.basename(fa)
    # the read-ahead thread samples the third file: the same bytes
    rc, out, p = _trac(world, "read_ahead", "HIP_MET_PREP", "1", "MET_DX", "2", "MET_SX", "2", "HIP_MET_PREFETCH", "1", exact=True)
    assert rc == 0 and "Meteo data from the read-ahead" in out, out[-3000:]
    for fa, fp in zip(_atm_files(a), _atm_files(p)):
        assert open(fa, "rb").read() == open(fp, "rb").read(), os.path.basename(fa)
    rc, out, c = _trac(world, "unsampled", exact=True)
    assert rc == 0 and open(_atm_files(a)[-1], "rb").read() != open(_atm_files(c)[-1], "rb").read()
    rc, out, _ = _trac(world, "refused", "MET_DX", "2")
    assert rc != 0 and "HIP_MET_PREP" in out and "MET_DX" in out, out[-2000:]
