"""module_oh_chem (src/mptrac.c:5351-5434) on the device against tests/refchem.py, with the temperature and the OH
value at each particle from the oracle's module_meteo; its place in the time step and the multi-step launches."""
import numpy as np
import pytest

import cases
import refchem
import refclim
from mptrac_amd import hip
from mptrac_amd.ctl import ctl_from_quantities
from mptrac_amd.synth import synthetic_particles
from oracle import binding as B

pytestmark = pytest.mark.gpu

NAMES = ("m", "vmr", "mloss_oh", "loss_rate")
OH = refclim.synthetic_zonal_mean(8, scale=1e-12)
MIXES = [(1, (3.5e-12, 0.0, 0.0, 0.0))] + [PRE for PRE in refchem.PRESETS.values()]


def _case(n, coord_type, beta, reaction, c, seed=4):
    ctl, clim, m0, m1, _ = cases.make_case("meteo", n=10)
    atm = synthetic_particles(n, seed=seed, quantities=NAMES, time=1800.0)
    atm["q"][0] = 1.0 + atm["lat"] / 180.0
    atm["q"][1] = 2e-9 * (1.0 + 0.5 * np.cos(np.radians(atm["lon"])))
    atm["q"][2:] = 0.0
    ctl = dict(cases.BASE, **ctl_from_quantities(NAMES), oh_chem_beta=beta, met_coord_type=coord_type,
               met_utm_ref_lat=48.15, met_utm_ref_lon=371.57, oh_chem_reaction=reaction, oh_chem=c)
    if coord_type == 1:
        m0.coord_type = m1.coord_type = 1
    return ctl, clim + ({"oh": OH},), m0, m1, atm


def _t_oh(ctl, clim, m0, m1, time, p, lon, lat):
    """temperature and OH at the particles: the oracle's module_meteo (quantities t, oh)"""
    names = ("t", "oh")
    octl = {k: v for k, v in ctl.items() if not k.startswith("qnt_")}
    octl.update(ctl_from_quantities(names))
    atm = {"time": time.copy(), "p": p.copy(), "lon": lon.copy(), "lat": lat.copy(), "q": np.zeros((2, len(time)))}
    o = B.Oracle(octl, clim, m0, m1, atm)
    o.module("meteo")
    r = o.state()
    return r["q"][0], r["q"][1]


def _idx(ctl):
    return {"m": ctl["qnt_m"], "vmr": ctl["qnt_vmr"], "mloss_oh": ctl["qnt_mloss_oh"], "loss_rate": ctl["qnt_loss_rate"]}


def single_module(coord_type, beta, reaction, c, mode="numpy", n=3000):
    """(device quantities, refchem quantities, dt) after module_timesteps + module_oh_chem at a day-and-night mix of
    times; every fifth particle is released later (dt = 0)."""
    ctl, clim, m0, m1, atm = _case(n, coord_type, beta, reaction, c)
    # (inside the two snapshots; day and night come from the longitudes)
    atm["time"][:] = 60.0 * (np.arange(n) % 40) + 7.0 * (np.arange(n) % 3)
    t = 2520.0
    atm["time"][::5] = 3000.0                      # not released yet: dt = 0
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    s.timesteps_init(atm["time"].min(), atm["time"].max())
    s.module("timesteps", t)
    s.module("oh_chem", t)
    g = s.state()
    dt = s.get_cache()["dt"]
    s.close()
    tt, oh = _t_oh(ctl, clim, m0, m1, atm["time"], atm["p"], atm["lon"], atm["lat"])
    ref = refchem.apply(atm["q"].copy(), _idx(ctl), reaction, c, atm["p"], tt, oh, dt, mode)
    return g, ref, dt, atm


def errors(g, ref, atm):
    """relative errors of m, vmr, mloss_oh, loss_rate; mloss_oh = m (1 - aux) relative to the initial mass (where
    dt rate is tiny 1 - aux cancels, in the reference as here)"""
    out = []
    for k in range(4):
        scale = atm["q"][0] if NAMES[k] == "mloss_oh" else np.abs(ref[k])
        out.append(float(np.max(np.abs(g["q"][k] - ref[k]) / np.maximum(scale, 1e-300))))
    return out


@pytest.mark.parametrize("coord_type", (0, 1))
@pytest.mark.parametrize("beta", (0.0, 0.6))
@pytest.mark.parametrize("mix", range(len(MIXES)))
def test_single_module_against_refchem(coord_type, beta, mix):
    reaction, c = MIXES[mix]
    g, ref, dt, atm = single_module(coord_type, beta, reaction, c)
    assert (dt == 0).sum() > 100 and (dt != 0).sum() > 1000
    off = dt == 0
    assert np.array_equal(g["q"][:, off], atm["q"][:, off])          # untouched
    assert np.array_equal(g["p"], atm["p"]) and np.array_equal(g["lon"], atm["lon"])
    assert np.mean(g["q"][0][~off] < atm["q"][0][~off]) > 0.9       # the chemistry acted
    for k, err in enumerate(errors(g, ref, atm)):
        assert err <= 1e-12, (NAMES[k], err)


def test_refused_without_table_or_mass():
    ctl, clim, m0, m1, atm = _case(100, 0, 0.0, 3, refchem.PRESETS["SO2"][1])
    s = hip.Simulation(ctl, clim[:3], m0, m1, atm)
    with pytest.raises(hip.MphipError, match="OH climatology was not uploaded"):
        s.module("oh_chem", 1800.0)
    s.close()
    names = ("loss_rate",)
    atm = synthetic_particles(100, seed=1, quantities=names, time=100.0)
    s = hip.Simulation(dict(ctl, **ctl_from_quantities(names), qnt_m=-1, qnt_vmr=-1, qnt_mloss_oh=-1), clim, m0, m1,
                       atm)
    with pytest.raises(hip.MphipError, match="Module needs quantity mass or volume mixing ratio!"):
        s.module("oh_chem", 1800.0)
    s.close()
    with pytest.raises(hip.MphipError, match="OH_CHEM_REACTION"):
        hip.Simulation(dict(ctl, oh_chem_reaction=4), clim, m0, m1, synthetic_particles(10, seed=1, quantities=NAMES))


C3_EXTRA = dict(tdec_trop=259200.0, tdec_strat=259200.0, dry_depo_vdep=0.15,
                wet_depo_ic_a=1e-4, wet_depo_ic_b=0.8, wet_depo_bc_a=5e-5, wet_depo_bc_b=0.6)


QB = ("m", "rp", "rhop", "vmr", "loss_rate", "mloss_oh", "mloss_decay")     # (b): quantity rows


class MeteoProbe:
    """temperature and OH at given positions from ONE oracle whose particle arrays (numpy views) are refilled"""

    def __init__(self, ctl, clim, m0, m1, n):
        octl = {k: v for k, v in ctl.items() if not k.startswith("qnt_")}
        octl.update(ctl_from_quantities(("t", "oh")))
        z = np.zeros(n)
        self.o = B.Oracle(octl, clim, m0, m1, {"time": z, "p": z + 500.0, "lon": z, "lat": z, "q": np.zeros((2, n))})

    def __call__(self, time, p, lon, lat):
        o = self.o
        o.time[:], o.p[:], o.lon[:], o.lat[:] = time, p, lon, lat
        o.module("meteo")
        return o.q[0].copy(), o.q[1].copy()


def _stepping(oh_on, n=4000, steps=20):
    ctl, clim, m0, m1, atm = cases.make_case("conv_sedi", n=n, quantities=QB)
    ctl.update(C3_EXTRA)
    if oh_on:
        ctl.update(oh_chem_reaction=3, oh_chem=refchem.PRESETS["SO2"][1])
    s = hip.Simulation(ctl, clim + ({"oh": OH},), m0, m1, atm)
    s.timesteps_init(atm["time"].min(), atm["time"].max())
    out = []
    for t in cases.step_times(s.ctl)[:steps]:
        s.run_timestep(t)
        out.append((t, s.state(), s.get_cache()))
    s.close()
    return ctl, clim, m0, m1, out


def test_oh_chemistry_moves_nothing_and_draws_nothing():
    """With and without the chemistry: positions, uvwp and the random-number counter are the same bits after every
    step.  Per step, the run with it has: mass = mass of the step before x decay, OH, wet and dry factors (in that
    order); mloss_oh = the one before + the mass after decay x (1 - OH factor); loss_rate = the run without it + the OH
    rate.  The OH factor and rate from refchem at the step's end state, the others from the run without it."""
    ctl, clim, m0, m1, on = _stepping(True)
    _, _, _, _, off = _stepping(False)
    iM, iL, iO, iD = QB.index("m"), QB.index("loss_rate"), QB.index("mloss_oh"), QB.index("mloss_decay")
    for (t, a, ca), (_, b, cb) in zip(on, off):
        for k in ("time", "p", "lon", "lat", "uvwp"):
            assert np.array_equal(a[k], b[k]), (t, k)
        assert ca["rng_ctr"] == cb["rng_ctr"]
    probe = MeteoProbe(ctl, clim + ({"oh": OH},), m0, m1, len(on[0][1]["time"]))
    for j in range(1, len(on)):
        t, a, ca = on[j]
        prev_on, prev_off, now_off = on[j - 1][1], off[j - 1][1], off[j][1]
        tt, oh = probe(a["time"], a["p"], a["lon"], a["lat"])
        mo_prev, mo_now = prev_off["q"][iM], now_off["q"][iM]
        ok = mo_prev != 0
        other = np.divide(mo_now, mo_prev, out=np.ones_like(mo_prev), where=ok)
        decay = 1.0 - np.divide(now_off["q"][iD] - prev_off["q"][iD], mo_prev, out=np.zeros_like(mo_prev), where=ok)
        dt = a["time"] - prev_on["time"]          # (the step's dt: the particle's time moved by it)
        fr = [refchem.factor(3, refchem.PRESETS["SO2"][1], a["p"][i], tt[i], oh[i], dt[i]) if dt[i] != 0 else (1.0, 0.0)
              for i in range(len(tt))]
        fac = np.array([f[0] for f in fr])
        rate = np.array([f[1] for f in fr])
        expect = prev_on["q"][iM] * other * fac
        err = np.max(np.abs(a["q"][iM] - expect) / np.maximum(np.abs(expect), 1e-300))
        assert err <= 1e-10, ("m", t, err)
        expect = prev_on["q"][iO] + prev_on["q"][iM] * decay * (1 - fac)
        err = np.max(np.abs(a["q"][iO] - expect) / prev_on["q"][iM])
        assert err <= 1e-10, ("mloss_oh", t, err)
        expect = now_off["q"][iL] + rate
        err = np.max(np.abs(a["q"][iL] - expect) / np.maximum(np.abs(expect), 1e-300))
        assert err <= 1e-10, ("loss_rate", t, err)
    assert np.mean(on[-1][1]["q"][iO] > 0) > 0.9
    assert np.mean(on[-1][1]["q"][iM] < off[-1][1]["q"][iM]) > 0.9


def test_multi_step_equals_single_steps():
    """run_timesteps with the chemistry gives the bits of single run_timestep calls (module_oh_chem is a launch of its
    own, so the steps go one by one: one step launch, the chemistry and the deposition launch per step)."""
    ctl, clim, m0, m1, atm = cases.make_case("conv_sedi", n=3000, quantities=("m", "rp", "rhop", "vmr", "loss_rate",
                                                                              "mloss_oh"))
    ctl.update(C3_EXTRA, oh_chem_reaction=3, oh_chem=refchem.PRESETS["CO"][1])
    res = []
    for multi in (True, False):
        s = hip.Simulation(ctl, clim + ({"oh": OH},), m0, m1, atm)
        s.timesteps_init(atm["time"].min(), atm["time"].max())
        times = cases.step_times(s.ctl)[:20]
        s.run_timestep(times[0])
        s.profile_begin()
        if multi:
            s.run_timesteps(times[1], len(times) - 1)
        else:
            for t in times[1:]:
                s.run_timestep(t)
        res.append((s.state(), s.get_cache()["rng_ctr"], s.profile_end()[0]))
        s.close()
    (a, ra, la), (b, rb, lb) = res
    assert ra == rb and la == lb >= 19
    for k in ("time", "p", "lon", "lat", "q", "uvwp"):
        assert np.array_equal(a[k], b[k]), k


def test_order_against_mixing():
    """C5's module set (module_sort, module_mixing, decay, wet and dry deposition, the movers) with the chemistry, the
    steps where the mixing is due included: the oracle driven module by module in orc_run_timestep's order
    (oracle/mptrac_oracle.c:1735-1785) with refchem inserted after module_mixing and before module_wet_depo."""
    names = cases.QUANTITIES + ("mloss_oh",)
    ctl, clim, m0, m1, atm = cases.make_case("full", n=4000, quantities=names)
    ctl.update(oh_chem_reaction=3, oh_chem=refchem.PRESETS["SO2"][1])
    clim = clim + ({"oh": OH},)
    o = B.Oracle(ctl, clim, m0, m1, atm)
    o.timesteps_init()
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    s.timesteps_init(atm["time"].min(), atm["time"].max())
    probe = MeteoProbe(ctl, clim, m0, m1, len(atm["time"]))
    idx = {"m": ctl["qnt_m"], "vmr": ctl["qnt_vmr"], "mloss_oh": ctl["qnt_mloss_oh"], "loss_rate": ctl["qnt_loss_rate"]}
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
        tt, oh = probe(o.time, o.p, o.lon, o.lat)
        refchem.apply(o.q, idx, 3, refchem.PRESETS["SO2"][1], o.p, tt, oh, o.dt)
        o.module("wet_depo")
        o.module("dry_depo")
    assert mixed >= 3 and len(times) >= 20
    g, r = s.state(), o.state()
    s.close()
    assert np.array_equal(g["time"], r["time"])
    for k in ("lon", "lat", "p"):
        assert cases.rel_err(g[k], r[k]) <= 1e-10, (k, cases.rel_err(g[k], r[k]))
    for k, name in enumerate(names):
        scale = np.maximum(np.abs(r["q"][k]), 1e-300) if name != "mloss_oh" else np.abs(r["q"][0])
        err = np.max(np.abs(g["q"][k] - r["q"][k]) / scale)
        assert err <= 1e-10, (name, err)
    assert np.mean(r["q"][names.index("mloss_oh")] > 0) > 0.9
