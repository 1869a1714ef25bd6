"""module_tracer_chem at full size: BASELINE configs[2] (C3: 10^7 particles, 721 x 361 x 137) with the four trace gases
(and Csf6), 20 steps in one mphip_run_timesteps call, against the oracle on a subsample with tests/reftracer.py behind
every step."""
import numpy as np
import pytest

import cases
import reftracer
from mptrac_amd import hip
from mptrac_amd.ctl import ctl_from_quantities
from oracle import binding as B
from test_gpu_tracer_chem import PHOTO, SPECIES, Probe, _clims, _idx, rel

pytestmark = pytest.mark.gpu


def add_o3c(met):
    """a total ozone column over the whole range of the photolysis table and beyond"""
    lam = np.radians(met.lon)[:, None]
    phi = np.radians(met.lat)[None, :]
    amp = met.time / 3600.0 * 0.01
    met.f2["o3c"] = np.ascontiguousarray(300.0 + 60.0 * np.sin(phi) + (15.0 + amp) * np.cos(lam), dtype=np.float32)


def c3_inputs(n, n_steps):
    import bench
    ctl, clim, met0, met1, atm, _, _ = bench.build_inputs("C3", 0, 1, n_steps + 1, particles=n)
    names = ("m", "rp", "rhop") + SPECIES + ("Csf6",)
    q = np.zeros((len(names), n))
    q[:3] = atm["q"][:3]
    rng = np.random.default_rng(17)
    for k in range(3, len(names)):
        q[k] = (1.0 + 0.1 * k) * 1e-10 * rng.uniform(0.5, 1.5, n)
    atm["q"] = q
    atm["p"][::3] = 10.0 ** rng.uniform(-0.5, 2.0, atm["p"][::3].size)      # a third in the stratosphere
    ctl.update(ctl_from_quantities(names), tracer_chem=1)
    for m in (met0, met1):
        add_o3c(m)
    return ctl, clim, met0, met1, atm, names


def test_c3_at_1e7_with_tracer_chemistry_against_the_oracle_subsample():
    n, n_steps = 10 ** 7, 20
    ctl, clim, met0, met1, atm, names = c3_inputs(n, n_steps)
    dclim, oclim = _clims(clim)
    s = hip.Simulation(ctl, dclim, met0, met1, atm)
    s.timesteps_init(0.0, 0.0)
    dt = s.ctl.dt_mod
    s.run_timestep(0.0)
    s.run_timesteps(dt, n_steps)
    g = s.state()
    s.close()
    pick = np.random.default_rng(20261016).choice(n, 3000, replace=False)
    sub = {k: (v[pick].copy() if k != "q" else v[:, pick].copy()) for k, v in atm.items()}
    o = B.Oracle(ctl, oclim, met0, met1, sub, ip_global=pick, np_global=n)
    o.timesteps_init()
    probe = Probe(ctl, oclim, met0, met1, len(pick))
    idx = _idx(ctl)
    for k in range(n_steps + 1):
        o.run_timestep(k * dt)          # (C3 has no module behind the chemistry's place)
        f = probe(o.time, o.p, o.lon, o.lat)
        reftracer.apply(o.q, idx, PHOTO, o.time, o.p, o.lon, o.lat, f["t"], f["o1d"], f["o3c"], o.dt)
    assert np.array_equal(g["time"][pick], o.time)
    for k, ref in (("lon", o.lon), ("lat", o.lat), ("p", o.p)):
        assert cases.rel_err(g[k][pick], ref) <= 1e-10, k
    for k, name in enumerate(names):
        assert rel(g["q"][k][pick], o.q[k]) <= 1e-10, name
        if name in SPECIES:
            assert np.mean(g["q"][k][pick] < sub["q"][k]) > 0.9, name
    assert np.array_equal(g["q"][names.index("Csf6")], atm["q"][names.index("Csf6")])
