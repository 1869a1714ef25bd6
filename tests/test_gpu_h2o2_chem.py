"""module_chem_grid and module_h2o2_chem on the device against tests/refh2o2.py (lwc, rwc, t and H2O2 at each particle
from the oracle's module_meteo, the cell-centre temperature from orc_intpol_met_time_3d); their place in the time step
behind module_mixing and around module_oh_chem, the multi-step launches, the refusals."""
import ctypes as C

import numpy as np
import pytest

import cases
import refchem
import refclim
import refh2o2
from mptrac_amd import hip
from mptrac_amd.ctl import ctl_from_quantities
from mptrac_amd.synth import FIELDS_3D, synthetic_particles
from oracle import binding as B

pytestmark = pytest.mark.gpu

OH = refclim.synthetic_zonal_mean(8, scale=1e-12)
H2O2 = refclim.synthetic_zonal_mean(9, scale=1e-9)
SO2_OH = refchem.PRESETS["SO2"][1]
GRID = dict(chemgrid_nx=36, chemgrid_ny=18, chemgrid_nz=6, chemgrid_lon0=-180.0, chemgrid_lon1=180.0,
            chemgrid_lat0=-90.0, chemgrid_lat1=90.0, chemgrid_z0=0.0, chemgrid_z1=18.0)
DEFAULT_GRID = dict(chemgrid_nx=360, chemgrid_ny=180, chemgrid_nz=1, chemgrid_lon0=-180.0, chemgrid_lon1=180.0,
                    chemgrid_lat0=-90.0, chemgrid_lat1=90.0, chemgrid_z0=-5.0, chemgrid_z1=85.0)
FULL = ("m", "vmr", "Cx", "mloss_h2o2", "loss_rate")


def _case(n, names, grid=GRID, seed=5, nens=0, **kw):
    ctl, clim, m0, m1, _ = cases.make_case("meteo", n=10)
    atm = synthetic_particles(n, seed=seed, quantities=names, time=1800.0)
    rng = np.random.default_rng(seed)
    atm["p"][:] = 1000.0 * np.exp(-rng.uniform(0.0, 1.6, n))      # (the synthetic clouds fill the lowest levels)
    q = atm["q"]
    q[:] = 0.0
    for k, name in enumerate(names):
        if name == "m":
            q[k] = 1e7 * (1.0 + atm["lat"] / 180.0)
        elif name == "vmr":
            q[k] = 2e-9 * (1.0 + 0.5 * np.cos(np.radians(atm["lon"])))
        elif name == "Cx":
            q[k] = 10.0 ** rng.uniform(-13.0, -6.0, n)               # below and above the threshold of the correction
        elif name == "ens":
            q[k] = np.arange(n) % max(nens, 1)
    ctl = dict(cases.BASE, **ctl_from_quantities(names), h2o2_chem_reaction=1, molmass=64.066, nens=nens, **grid)
    ctl.update(kw)
    return ctl, clim + ({"h2o2": H2O2, "oh": OH},), m0, m1, atm


def _idx(ctl):
    return {"m": ctl.get("qnt_m", -1), "vmr": ctl.get("qnt_vmr", -1), "Cx": ctl.get("qnt_Cx", -1),
            "mloss_h2o2": ctl.get("qnt_mloss_h2o2", -1), "mloss_oh": ctl.get("qnt_mloss_oh", -1),
            "loss_rate": ctl.get("qnt_loss_rate", -1), "ens": ctl.get("qnt_ens", -1)}


class Probe:
    """t, lwc, rwc, h2o2 and oh at given positions from ONE oracle (module_meteo), and the temperature at a point
    (orc_intpol_met_time_3d)"""
    NAMES = ("t", "lwc", "rwc", "h2o2", "oh")

    def __init__(self, ctl, clim, m0, m1, n):
        octl = {k: v for k, v in ctl.items() if not k.startswith("qnt_")}
        octl.update(ctl_from_quantities(self.NAMES))
        z = np.zeros(n)
        self.o = B.Oracle(octl, clim, m0, m1, {"time": z, "p": z + 500.0, "lon": z, "lat": z,
                                                "q": np.zeros((len(self.NAMES), n))})

    def __call__(self, time, p, lon, lat):
        o = self.o
        o.time[:], o.p[:], o.lon[:], o.lat[:] = time, p, lon, lat
        o.module("meteo")
        return {k: o.q[i].copy() for i, k in enumerate(self.NAMES)}

    def temp_at(self, t, p, lon, lat):
        v = C.c_double()
        o = self.o
        o.lib.orc_intpol_met_time_3d(C.byref(o.met[0]), C.byref(o.met[1]), FIELDS_3D.index("t"), t, p, lon, lat,
                                     C.byref(v))
        return v.value


def single_h2o2(names, mode="numpy", n=3000, **kw):
    """(device state, refh2o2 quantities, dt, atm) after module_timesteps + module_h2o2_chem; every fifth particle is
    released later (dt = 0)"""
    ctl, clim, m0, m1, atm = _case(n, names, **kw)
    atm["time"][:] = 60.0 * (np.arange(n) % 40) + 7.0 * (np.arange(n) % 3)
    atm["time"][::5] = 3000.0
    t = 2520.0
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    s.timesteps_init(atm["time"].min(), atm["time"].max())
    s.module("timesteps", t)
    s.module("h2o2_chem", t)
    g = s.state()
    dt = s.get_cache()["dt"]
    s.close()
    f = Probe(ctl, clim, m0, m1, n)(atm["time"], atm["p"], atm["lon"], atm["lat"])
    ref = refh2o2.h2o2_chem(atm["q"].copy(), _idx(ctl), atm["p"], f["t"], f["lwc"], f["rwc"], f["h2o2"], dt, mode)
    return g, ref, dt, atm, f


def single_grid(names, mode="numpy", n=4000, t=1800.0, **kw):
    """(device state, refh2o2 quantities, cells, atm) after module_chem_grid at t; a tenth of the particles lies outside
    the time window"""
    ctl, clim, m0, m1, atm = _case(n, names, **kw)
    atm["time"][::10] = t - 400.0
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    s.module("chem_grid", t)
    g = s.state()
    s.close()
    probe = Probe(ctl, clim, m0, m1, n)
    ref = atm["q"].copy()
    cell, _ = refh2o2.chem_grid(ctl, ref, _idx(ctl), t, atm["time"], atm["p"], atm["lon"], atm["lat"], probe.temp_at,
                                mode)
    return g, ref, cell, atm


def rel(a, b, scale=None):
    scale = np.abs(b) if scale is None else scale
    return float(np.max(np.abs(a - b) / np.maximum(scale, 1e-300), initial=0.0))


H2O2_SETS = [FULL, ("m", "Cx"), ("m", "mloss_h2o2"), ("vmr",), ("vmr", "Cx"), ("m", "vmr", "Cx", "ens")]


@pytest.mark.parametrize("names", H2O2_SETS, ids=["+".join(x) for x in H2O2_SETS])
def test_h2o2_chem_against_restatement(names):
    g, ref, dt, atm, f = single_h2o2(names, nens=3 if "ens" in names else 0)
    inside = (f["lwc"] > 0) | (f["rwc"] > 0)
    assert (dt == 0).sum() > 100 and (inside & (dt != 0)).sum() > 300 and (~inside & (dt != 0)).sum() > 300
    untouched = (dt == 0) | ~inside
    assert np.array_equal(g["q"][:, untouched], atm["q"][:, untouched])
    first = 0 if "m" in names else names.index("vmr")
    assert np.mean(g["q"][first][~untouched] < atm["q"][first][~untouched]) > 0.9      # the chemistry acted
    if "Cx" in names:
        cx = atm["q"][names.index("Cx")][~untouched]
        assert (cx > refh2o2.low()).sum() > 50 and (cx < refh2o2.low()).sum() > 50
    for k, name in enumerate(names):
        scale = atm["q"][0] if name == "mloss_h2o2" else None
        assert rel(g["q"][k], ref[k], scale) <= 1e-12, name


@pytest.mark.parametrize("grid,nens", [(GRID, 0), (DEFAULT_GRID, 0), (GRID, 4)], ids=["coarse", "default", "ensemble"])
@pytest.mark.parametrize("sums", ("ordered", "atomic"))
def test_chem_grid_against_serial_sums(grid, nens, sums):
    names = ("m", "Cx", "ens") if nens else ("m", "vmr", "Cx")
    ctl, clim, m0, m1, atm = _case(4000, names, grid=grid, nens=nens)
    t = 1800.0
    atm["time"][::10] = t - 400.0
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    if sums == "atomic":
        s.set_option("deterministic_sums", 0)
    s.module("chem_grid", t)
    g = s.state()
    s.close()
    probe = Probe(ctl, clim, m0, m1, len(atm["time"]))
    ref = atm["q"].copy()
    cell, mass = refh2o2.chem_grid(ctl, ref, _idx(ctl), t, atm["time"], atm["p"], atm["lon"], atm["lat"],
                                   probe.temp_at)
    k = names.index("Cx")
    inside = cell >= 0
    assert inside.sum() > 2000 and (~inside).sum() > 300
    assert np.array_equal(g["q"][k][~inside], atm["q"][k][~inside])          # outside: Cx kept
    assert rel(g["q"][k], ref[k]) <= 1e-12
    if grid is GRID:                                                          # many particles share a cell
        assert np.bincount(cell[inside]).max() > 3
    for j, name in enumerate(names):
        if name != "Cx":
            assert np.array_equal(g["q"][j], atm["q"][j]), name


def test_chem_grid_without_mass_or_cx_does_nothing():
    for names in (("vmr", "Cx"), ("m", "vmr")):
        ctl, clim, m0, m1, atm = _case(500, names)
        s = hip.Simulation(ctl, clim, m0, m1, atm)
        s.module("chem_grid", 1800.0)
        g = s.state()
        s.close()
        assert np.array_equal(g["q"], atm["q"])


def test_refusals():
    ctl, clim, m0, m1, atm = _case(200, FULL)
    s = hip.Simulation(ctl, clim[:3] + ({"oh": OH},), m0, m1, atm)
    with pytest.raises(hip.MphipError, match="H2O2 climatology was not uploaded"):
        s.module("h2o2_chem", 1800.0)
    s.close()
    for bad in (dict(molmass=0.0), dict(molmass=-1.0)):
        s = hip.Simulation(dict(ctl, **bad), clim, m0, m1, atm)
        with pytest.raises(hip.MphipError, match="Molar mass is not defined!"):
            s.module("chem_grid", 1800.0)
        s.close()
    for bad in (dict(chemgrid_nx=0), dict(chemgrid_nz=0), dict(chemgrid_lat1=-90.0), dict(chemgrid_z1=0.0)):
        s = hip.Simulation(dict(ctl, **bad), clim, m0, m1, atm)
        with pytest.raises(hip.MphipError, match="invalid chemistry grid"):
            s.module("chem_grid", 1800.0)
        with pytest.raises(hip.MphipError, match="invalid chemistry grid"):
            s.run_timestep(1800.0)
        s.close()
    names = ("loss_rate",)
    s = hip.Simulation(dict(ctl, **ctl_from_quantities(names), qnt_m=-1, qnt_vmr=-1, qnt_Cx=-1, qnt_mloss_h2o2=-1),
                       clim, m0, m1, synthetic_particles(100, seed=1, quantities=names, time=100.0))
    with pytest.raises(hip.MphipError, match="Module needs quantity mass or volume mixing ratio!"):
        s.module("h2o2_chem", 1800.0)
    s.close()
    # meteo without cloud water
    c2, cl2, n0, n1, a2 = cases.make_case("conv_sedi", n=100, quantities=FULL,
                                          fields=("u", "v", "w", "t", "ps", "pbl", "cape", "cin", "pel"))
    s = hip.Simulation(dict(ctl, **ctl_from_quantities(FULL)), clim, n0, n1, a2)
    s.timesteps_init(a2["time"].min(), a2["time"].max())
    s.module("timesteps", 1800.0)
    with pytest.raises(hip.MphipError, match="t, lwc and rwc were not uploaded"):
        s.module("h2o2_chem", 1800.0)
    s.close()


STEP_NAMES = ("m", "rp", "rhop", "vmr", "loss_rate", "mloss_oh", "mloss_h2o2", "Cx")


def _stepping(chem, n=4000, steps=20, multi=False):
    ctl, clim, m0, m1, atm = cases.make_case("conv_sedi", n=n, quantities=STEP_NAMES)
    atm["q"][STEP_NAMES.index("m")] = 1e7 * (1.0 + atm["lat"] / 180.0)
    atm["q"][STEP_NAMES.index("Cx")] = 0.0
    atm["p"][::2] = 700.0 + 250.0 * np.random.default_rng(3).uniform(size=atm["p"][::2].size)   # (into the clouds)
    ctl.update(molmass=64.066, **GRID)
    if chem:
        ctl.update(oh_chem_reaction=3, oh_chem=SO2_OH, h2o2_chem_reaction=1)
    s = hip.Simulation(ctl, clim + ({"oh": OH, "h2o2": H2O2},), m0, m1, atm)
    s.timesteps_init(atm["time"].min(), atm["time"].max())
    times = cases.step_times(s.ctl)[:steps]
    out = []
    if multi:
        s.run_timestep(times[0])
        s.run_timesteps(times[1], len(times) - 1)
        out.append((times[-1], s.state(), s.get_cache()))
    else:
        for t in times:
            s.run_timestep(t)
            out.append((t, s.state(), s.get_cache()))
    s.close()
    return ctl, atm, out


def test_chemistry_moves_nothing_draws_nothing_and_closes_mass():
    """With and without OH + H2O2 + Cx: positions, uvwp and the random-number counter are the same bits after every
    step; with them m + mloss_oh + mloss_h2o2 = m0, and both chemistries acted."""
    ctl, atm, on = _stepping(True)
    _, _, off = _stepping(False)
    iM, iO, iH, iC = (STEP_NAMES.index(k) for k in ("m", "mloss_oh", "mloss_h2o2", "Cx"))
    m0 = atm["q"][iM]
    for (t, a, ca), (_, b, cb) in zip(on, off):
        for k in ("time", "p", "lon", "lat", "uvwp"):
            assert np.array_equal(a[k], b[k]), (t, k)
        assert ca["rng_ctr"] == cb["rng_ctr"]
        closure = a["q"][iM] + a["q"][iO] + a["q"][iH]
        assert rel(closure, m0) <= 1e-12, t
        assert np.array_equal(b["q"][iM], m0) and not b["q"][iC].any()
    last = on[-1][1]["q"]
    assert np.mean(last[iO] > 0) > 0.9 and (last[iH] > 0).sum() > 100 and np.mean(last[iC] > 0) > 0.5


def test_multi_step_equals_single_steps():
    _, _, single = _stepping(True)
    _, _, multi = _stepping(True, multi=True)
    a, b = single[-1][1], multi[-1][1]
    assert single[-1][2]["rng_ctr"] == multi[-1][2]["rng_ctr"]
    for k in ("time", "p", "lon", "lat", "q", "uvwp"):
        assert np.array_equal(a[k], b[k]), k


def test_order_against_mixing_and_oh():
    """C5's module set (module_sort, module_mixing, decay, wet and dry deposition, the movers) with OH, H2O2 and Cx: the
    oracle driven module by module in orc_run_timestep's order with refh2o2.chem_grid (after module_mixing: Cx from the
    mixed masses), refchem (OH) and refh2o2.h2o2_chem (after OH) before module_wet_depo."""
    names = cases.QUANTITIES + ("mloss_oh", "mloss_h2o2", "Cx")
    ctl, clim, m0, m1, atm = cases.make_case("full", n=4000, quantities=names)
    atm["q"][names.index("m")] *= 1e7
    atm["p"][::2] = 700.0 + 250.0 * np.random.default_rng(3).uniform(size=atm["p"][::2].size)   # (into the clouds)
    ctl.update(oh_chem_reaction=3, oh_chem=SO2_OH, h2o2_chem_reaction=1, molmass=64.066, **GRID)
    clim = clim + ({"oh": OH, "h2o2": H2O2},)
    o = B.Oracle(ctl, clim, m0, m1, atm)
    o.timesteps_init()
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    s.timesteps_init(atm["time"].min(), atm["time"].max())
    probe = Probe(ctl, clim, m0, m1, len(atm["time"]))
    idx = _idx(ctl)
    c = o.ctl
    times = cases.step_times(c)
    mixed = 0
    for t in times:
        s.run_timestep(t)
        o.module("timesteps", t)
        if c.sort_dt > 0 and np.fmod(t, c.sort_dt) == 0:
            o.sort()
        o.module("position")
        o.module("advect")
        o.module("diff_turb")
        o.module("diff_meso")
        o.module("convection")
        o.module("sedi")
        o.module("position")
        o.q[c.qnt_loss_rate][o.dt != 0] = 0
        o.module("decay")
        if np.fmod(t, c.mixing_dt) == 0:
            o.module("mixing", t)
            mixed += 1
        refh2o2.chem_grid(ctl, o.q, idx, t, o.time, o.p, o.lon, o.lat, probe.temp_at)
        f = probe(o.time, o.p, o.lon, o.lat)
        refchem.apply(o.q, idx, 3, SO2_OH, o.p, f["t"], f["oh"], o.dt)
        refh2o2.h2o2_chem(o.q, idx, o.p, f["t"], f["lwc"], f["rwc"], f["h2o2"], o.dt)
        o.module("wet_depo")
        o.module("dry_depo")
    assert mixed >= 3 and len(times) >= 20
    g, r = s.state(), o.state()
    s.close()
    assert np.array_equal(g["time"], r["time"])
    for k in ("lon", "lat", "p"):
        assert cases.rel_err(g[k], r[k]) <= 1e-10, (k, cases.rel_err(g[k], r[k]))
    for k, name in enumerate(names):
        scale = np.abs(r["q"][0]) if name.startswith("mloss") else None
        assert rel(g["q"][k], r["q"][k], scale) <= 1e-10, name
    assert (r["q"][names.index("mloss_h2o2")] > 0).sum() > 100
    assert np.mean(r["q"][names.index("Cx")] > 0) > 0.5      # (GRID ends at 18 km)
