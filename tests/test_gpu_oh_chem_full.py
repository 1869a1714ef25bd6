"""module_oh_chem at full size and through the drop-in driver:
  (e) BASELINE configs[2] (C3: 10^7 particles, 721 x 361 x 137) with SO2's OH chemistry, 20 steps in one
      mphip_run_timesteps call, against the oracle on a subsample with tests/refchem.py behind every step;
  (f) `trac` with SPECIES SO2 and no OH_CHEM_REACTION key on MET_TYPE 1 files and a classic-netCDF OH table: the
      chemistry is on by default, the particle file carries mloss_oh, and the mass is closed."""
import os
import subprocess

import numpy as np
import pytest

import cases
import hostfiles as hf
import refchem
import refclim
from mptrac_amd import build, hip
from mptrac_amd.synth import synthetic_met, synthetic_particles
from oracle import binding as B
from test_gpu_oh_chem import MeteoProbe

pytestmark = pytest.mark.gpu
SO2 = refchem.PRESETS["SO2"]
OH = refclim.synthetic_zonal_mean(8, scale=1e-12)


def test_c3_at_1e7_with_so2_chemistry_against_the_oracle_subsample():
    import bench
    n, n_steps = 10 ** 7, 20
    ctl, clim, met0, met1, atm, _, _ = bench.build_inputs("C3", 0, 1, n_steps + 1, particles=n)
    ctl.update(oh_chem_reaction=SO2[0], oh_chem=SO2[1])
    clim = clim + ({"oh": OH},)
    s = hip.Simulation(ctl, clim, met0, met1, atm)
    s.timesteps_init(0.0, 0.0)
    dt = s.ctl.dt_mod
    s.run_timestep(0.0)
    s.run_timesteps(dt, n_steps)
    g = s.state()
    s.close()
    pick = np.random.default_rng(20261015).choice(n, 3000, replace=False)
    sub = {k: (v[pick].copy() if k != "q" else v[:, pick].copy()) for k, v in atm.items()}
    o = B.Oracle(ctl, clim, met0, met1, sub, ip_global=pick, np_global=n)
    o.timesteps_init()
    probe = MeteoProbe(ctl, clim, met0, met1, len(pick))
    idx = {"m": ctl["qnt_m"]}
    for k in range(n_steps + 1):
        o.run_timestep(k * dt)          # (C3 has no module behind the chemistry's place)
        tt, oh = probe(o.time, o.p, o.lon, o.lat)
        refchem.apply(o.q, idx, SO2[0], SO2[1], o.p, tt, oh, o.dt)
    assert np.array_equal(g["time"][pick], o.time)
    for k, ref in (("lon", o.lon), ("lat", o.lat), ("p", o.p)):
        assert cases.rel_err(g[k][pick], ref) <= 1e-10, k
    m = g["q"][ctl["qnt_m"]][pick]
    err = np.max(np.abs(m - o.q[ctl["qnt_m"]]) / np.abs(o.q[ctl["qnt_m"]]))
    assert err <= 1e-10, err
    assert np.mean(m < sub["q"][ctl["qnt_m"]]) > 0.9


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


def _trac(tmp, extra):
    _, trac = build.build_host()
    quant = ("m", "mloss_oh", "mloss_wet", "mloss_dry")
    metbase = os.path.join(tmp, "met")
    for k in range(3):
        m = synthetic_met("tiny", T0 + 3600.0 * k, 1.0 + 0.1 * k, fields=cases.PRESSURE_LEVEL_FIELDS)
        hf.write_met_bin(hf.met_filename(metbase, m.time), m)
    atm = synthetic_particles(3000, time=T0, quantities=quant)
    atm["q"][1:] = 0.0
    hf.write_atm_bin(os.path.join(tmp, "atm_in"), atm)
    _write_oh(os.path.join(tmp, "oh.nc"))
    keys = {"NQ": len(quant), "METBASE": metbase, "MET_TYPE": 1, "DT_MET": 3600, "DT_MOD": 180, "ADVECT": 2,
            "T_STOP": T0 + 7200.0, "ATM_TYPE": 1, "ATM_TYPE_OUT": 1, "ATM_BASENAME": "atm", "ATM_DT_OUT": 3600,
            "MET_DT_OUT": 0, "SPECIES": "SO2", "CLIM_OH_FILENAME": os.path.join(tmp, "oh.nc")}
    keys.update({"QNT_NAME[%d]" % i: q for i, q in enumerate(quant)})
    keys.update(extra)
    hf.write_ctl(os.path.join(tmp, "trac.ctl"), keys)
    open(os.path.join(tmp, "dirlist"), "w").write(tmp + "\n")
    r = subprocess.run([trac, os.path.join(tmp, "dirlist"), "trac.ctl", "atm_in"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    return atm, hf.read_atm_bin(os.path.join(tmp, "atm_2022_06_02_02_00_00.bin"), len(quant)), out


def test_trac_runs_species_so2_with_its_oh_chemistry(tmp_path):
    on_dir, off_dir = tmp_path / "on", tmp_path / "off"
    on_dir.mkdir()
    off_dir.mkdir()
    atm, on, out = _trac(str(on_dir), {})
    assert "OH_CHEM_REACTION = 3" in out
    m0 = atm["q"][0]
    total = on["q"][0] + on["q"][1] + on["q"][2] + on["q"][3]
    assert np.max(np.abs(total - m0) / m0) <= 1e-12
    assert np.mean(on["q"][1] > 0) > 0.9
    _, off, out = _trac(str(off_dir), {"OH_CHEM_REACTION": 0})
    assert "OH chemistry" not in out
    assert np.all(off["q"][1] == 0) and not np.array_equal(on["q"][0], off["q"][0])
    assert np.array_equal(on["lon"], off["lon"]) and np.array_equal(on["p"], off["p"])
