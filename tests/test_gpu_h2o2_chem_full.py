"""module_chem_grid and module_h2o2_chem at full size, over shards and through the drop-in driver:
  (g) BASELINE configs[2] (C3: 10^7 particles, 721 x 361 x 137, with cloud water) with SO2's OH chemistry, the H2O2
      chemistry and Cx on the default chemistry grid, 20 steps: positions against the oracle on a subsample with
      tests/refchem.py and tests/refh2o2.py behind every step, Cx of the last step against refh2o2.chem_grid over all
      10^7 particles;
  (h) two index-range shards with the all-reduce hook give the Cx of one context;
  (i) `trac` with SPECIES SO2 and Cx on MET_TYPE 1 files writes the Cx the restatement computes from its own output."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import cases
import hostfiles as hf
import refchem
import refh2o2
from mptrac_amd import build, hip
from mptrac_amd.synth import synthetic_met, synthetic_particles
from oracle import binding as B
from test_gpu_full_size import _ThreadAllreduce
from test_gpu_h2o2_chem import GRID, H2O2, OH, Probe

pytestmark = pytest.mark.gpu
SO2 = refchem.PRESETS["SO2"]


def _cells_vectorised(ctl, t, time, p, lon, lat):
    """refh2o2.cells for many particles at once (numpy)"""
    nx, ny, nz = ctl["chemgrid_nx"], ctl["chemgrid_ny"], ctl["chemgrid_nz"]
    dz = (ctl["chemgrid_z1"] - ctl["chemgrid_z0"]) / nz
    dlon = (ctl["chemgrid_lon1"] - ctl["chemgrid_lon0"]) / nx
    dlat = (ctl["chemgrid_lat1"] - ctl["chemgrid_lat0"]) / ny
    z = refh2o2.H0 * np.log(refh2o2.P0 / p)
    ok = ~((time < t - 0.5 * ctl["dt_mod"]) | (time > t + 0.5 * ctl["dt_mod"]) | (lon < ctl["chemgrid_lon0"])
           | (lon >= ctl["chemgrid_lon1"]) | (lat < ctl["chemgrid_lat0"]) | (lat >= ctl["chemgrid_lat1"])
           | (z < ctl["chemgrid_z0"]) | (z >= ctl["chemgrid_z1"]))
    ix = np.where(ok, (lon - ctl["chemgrid_lon0"]) / dlon, 0).astype(np.int64)
    iy = np.where(ok, (lat - ctl["chemgrid_lat0"]) / dlat, 0).astype(np.int64)
    iz = np.where(ok, (z - ctl["chemgrid_z0"]) / dz, 0).astype(np.int64)
    ok &= (ix < nx) & (iy < ny) & (iz < nz)
    return np.where(ok, (ix * ny + iy) * nz + iz, -1), ix, iy, iz


def _cx_reference(ctl, probe, t, time, p, lon, lat, m):
    cell, ix, iy, iz = _cells_vectorised(ctl, t, time, p, lon, lat)
    ok = cell >= 0
    mass = np.zeros(ctl["chemgrid_nx"] * ctl["chemgrid_ny"] * ctl["chemgrid_nz"])
    np.add.at(mass, cell[ok], m[ok])
    press, glon, glat, area, dz = refh2o2.grid_tables(ctl)
    cx = np.full(len(time), np.nan)
    table = {}
    for c in np.unique(cell[ok]):
        iz_, iy_, ix_ = c % ctl["chemgrid_nz"], (c // ctl["chemgrid_nz"]) % ctl["chemgrid_ny"], \
            c // (ctl["chemgrid_nz"] * ctl["chemgrid_ny"])
        temp = probe.temp_at(t, press[iz_], glon[ix_], glat[iy_])
        rho = 100. * press[iz_] / (refh2o2.RA * temp)
        table[c] = refh2o2.MA / ctl["molmass"] * mass[c] / (1e9 * rho * area[iy_] * dz)
    vals = np.array([table[c] for c in cell[ok]])
    cx[ok] = vals
    return cell, cx


def test_c3_at_1e7_with_oh_h2o2_and_cx_against_the_oracle_subsample():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import gpu_h2o2_chem_cost as cost
    n, n_steps = 10 ** 7, 20
    ctl, clim, met0, met1, atm = cost.so2_inputs("so2", n_steps + 1, n)
    iM, iC = ctl["qnt_m"], ctl["qnt_Cx"]
    s = hip.Simulation(ctl, clim, met0, met1, atm)
    s.timesteps_init(0.0, 0.0)
    dt = s.ctl.dt_mod
    pick = np.random.default_rng(20261016).choice(n, 3000, replace=False)
    sub = {k: (v[pick].copy() if k != "q" else v[:, pick].copy()) for k, v in atm.items()}
    o = B.Oracle(ctl, clim, met0, met1, sub, ip_global=pick, np_global=n)
    o.timesteps_init()
    probe = Probe(ctl, clim, met0, met1, len(pick))
    idx = {"m": iM, "Cx": iC}
    prev = None
    for k in range(n_steps + 1):
        t = k * dt
        s.run_timestep(t)
        g = s.state()
        o.run_timestep(t)                 # (C3 has no module behind the chemistry's place)
        o.q[iC] = g["q"][iC][pick]        # (Cx needs every particle: the device's, checked below)
        f = probe(o.time, o.p, o.lon, o.lat)
        refchem.apply(o.q, idx, SO2[0], SO2[1], o.p, f["t"], f["oh"], o.dt)
        refh2o2.h2o2_chem(o.q, idx, o.p, f["t"], f["lwc"], f["rwc"], f["h2o2"], o.dt)
        if k == n_steps:                  # Cx of this step: positions after it, masses before its chemistry
            cell, cx = _cx_reference(ctl, Probe(ctl, clim, met0, met1, 1), t, g["time"], g["p"], g["lon"], g["lat"],
                                     prev["q"][iM])
            inside = cell >= 0
            assert inside.sum() > n // 2
            err = np.max(np.abs(g["q"][iC][inside] - cx[inside]) / np.abs(cx[inside]))
            assert err <= 1e-12, err
        prev = g
    s.close()
    assert np.array_equal(g["time"][pick], o.time)
    for key, ref in (("lon", o.lon), ("lat", o.lat), ("p", o.p)):
        assert cases.rel_err(g[key][pick], ref) <= 1e-10, key
    m = g["q"][iM][pick]
    err = np.max(np.abs(m - o.q[iM]) / np.abs(o.q[iM]))
    assert err <= 1e-10, err
    assert np.mean(m < sub["q"][iM]) > 0.9


def test_two_shards_with_the_allreduce_give_the_cx_of_one_context():
    world, n = 2, 40000
    ctl, clim, m0, m1, atm = cases.make_case("conv_sedi", n=n, quantities=("m", "vmr", "Cx"))
    atm["q"][0] *= 1e7
    atm["q"][2] = 0.0
    ctl.update(oh_chem_reaction=3, oh_chem=SO2[1], h2o2_chem_reaction=1, molmass=64.066, **GRID)
    clim = clim + ({"oh": OH, "h2o2": H2O2},)
    one = hip.Simulation(ctl, clim, m0, m1, atm)
    one.timesteps_init(0.0, 0.0)
    times = cases.step_times(one.ctl)[:6]
    for t in times:
        one.run_timestep(t)
    ref = one.state()
    one.close()
    ar = _ThreadAllreduce(world)
    out, errors = [None] * world, []

    def rank_main(rank):
        try:
            lo, hi = hip.shard_range(n, rank, world)
            s = hip.Simulation(ctl, clim, m0, m1, atm, shard=(lo, hi))
            s.set_allreduce(ar.hook(rank))
            s.timesteps_init(0.0, 0.0)
            for t in times:
                s.run_timestep(t)
            out[rank] = (lo, hi, s.state())
            s.close()
        except BaseException as exc:      # noqa: BLE001
            errors.append((rank, repr(exc)))
            ar.barrier.abort()
    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert all(c >= len(times) for c in ar.calls)
    cx = np.concatenate([g["q"][2] for _, _, g in out])
    assert np.mean(ref["q"][2] > 0) > 0.5      # (GRID ends at 18 km)
    err = np.max(np.abs(cx - ref["q"][2]) / np.maximum(np.abs(ref["q"][2]), 1e-300))
    assert err <= 1e-14, err
    for k in ("lon", "lat", "p"):
        assert np.array_equal(np.concatenate([g[k] for _, _, g in out]), ref[k]), k


T0 = 707443200.0      # 2022-06-02 00:00 UTC


def _write_oh(path):
    from scipy.io import netcdf_file
    _, p, lat, vmr = OH
    with netcdf_file(path, "w", version=1) as f:
        f.createDimension("time", 12)
        f.createDimension("press", len(p))
        f.createDimension("lat", len(lat))
        f.createVariable("press", "d", ("press",))[:] = p
        f.createVariable("lat", "d", ("lat",))[:] = lat
        f.createVariable("OH", "d", ("time", "press", "lat"))[:] = vmr


def test_trac_writes_cx_of_species_so2(tmp_path):
    """Cx at the output time t from trac's own particle files: positions of the file at t, masses of the file one step
    earlier (module_chem_grid runs before the chemistry of the step), the grid of the control file."""
    _, trac = build.build_host()
    tmp = str(tmp_path)
    quant = ("m", "Cx", "mloss_oh")
    metbase = os.path.join(tmp, "met")
    mets = []
    for k in range(3):
        m = synthetic_met("tiny", T0 + 3600.0 * k, 1.0 + 0.1 * k, fields=cases.PRESSURE_LEVEL_FIELDS)
        hf.write_met_bin(hf.met_filename(metbase, m.time), m)
        mets.append(m)
    atm = synthetic_particles(3000, time=T0, quantities=quant)
    atm["q"][0] *= 1e9
    atm["q"][1:] = 0.0
    hf.write_atm_bin(os.path.join(tmp, "atm_in"), atm)
    _write_oh(os.path.join(tmp, "oh.nc"))
    keys = {"NQ": len(quant), "METBASE": metbase, "MET_TYPE": 1, "DT_MET": 3600, "DT_MOD": 180, "ADVECT": 2,
            "T_STOP": T0 + 3600.0, "ATM_TYPE": 1, "ATM_TYPE_OUT": 1, "ATM_BASENAME": "atm", "ATM_DT_OUT": 180,
            "MET_DT_OUT": 0, "SPECIES": "SO2", "CLIM_OH_FILENAME": os.path.join(tmp, "oh.nc"),
            "CHEMGRID_NX": 36, "CHEMGRID_NY": 18, "CHEMGRID_NZ": 6, "CHEMGRID_Z0": 0, "CHEMGRID_Z1": 18}
    keys.update({"QNT_NAME[%d]" % i: q for i, q in enumerate(quant)})
    hf.write_ctl(os.path.join(tmp, "trac.ctl"), keys)
    open(os.path.join(tmp, "dirlist"), "w").write(tmp + "\n")
    r = subprocess.run([trac, os.path.join(tmp, "dirlist"), "trac.ctl", "atm_in"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    assert "CHEMGRID_NX = 36" in out
    before = hf.read_atm_bin(os.path.join(tmp, "atm_2022_06_02_00_57_00.bin"), len(quant))
    after = hf.read_atm_bin(os.path.join(tmp, "atm_2022_06_02_01_00_00.bin"), len(quant))
    t = T0 + 3600.0
    ctl = dict(GRID, chemgrid_nx=36, chemgrid_ny=18, chemgrid_nz=6, chemgrid_z0=0.0, chemgrid_z1=18.0, dt_mod=180.0,
               molmass=64.066)
    probe = Probe(dict(cases.BASE), cases.load_clim_tropo() + ({"oh": OH, "h2o2": H2O2},), mets[1], mets[2], 1)
    cell, cx = _cx_reference(ctl, probe, t, after["time"], after["p"], after["lon"], after["lat"], before["q"][0])
    inside = cell >= 0
    assert inside.sum() > 1000
    err = np.max(np.abs(after["q"][1][inside] - cx[inside]) / np.abs(cx[inside]))
    assert err <= 1e-12, err
    assert np.mean(after["q"][2] > 0) > 0.9                    # (the OH chemistry ran as well)
