"""module_radio_decay on the device against tests/refradio.py: the module alone for each activity and all six, what it
must leave alone, DIRECTION -1, 20 steps against the oracle, multi-step launches, its place in the time step behind
module_decay, module_mixing, the OH and tracer chemistry and before the deposition, two shards with mixing, the
refusals of mphip_set_radio_decay, and C3 at 1e7 particles."""
import os
import sys
import threading

import numpy as np
import pytest

import cases
import refradio
import test_gpu_tracer_chem as TC
from mptrac_amd import hip
from mptrac_amd.ctl import ctl_from_quantities
from mptrac_amd.synth import synthetic_particles
from oracle import binding as B
from test_gpu_full_size import _ThreadAllreduce

pytestmark = pytest.mark.gpu

ACT = refradio.NAMES


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300), initial=0.0))


def _fill(atm, names, seed=7):
    """activities of 10 ... 1e6 Bq that vary between the particles (Rn-222 large against Pb-210: visible ingrowth)"""
    rng = np.random.default_rng(seed)
    n = len(atm["time"])
    for k, name in enumerate(names):
        if name in ACT:
            atm["q"][k] = 10.0 ** rng.uniform(1.0, 4.0, n) * (1e2 if name == "Arn222" else 1.0)


def _idx(names):
    return [list(names).index(x) if x in names else -1 for x in ACT]


def single(names, mode="numpy", n=100000, steps=1, direction=1):
    """(device state, restatement, dt, atm) after module_timesteps and `steps` calls of module_radio_decay on its dt;
    every fifth particle is not released yet (dt = 0)"""
    ctl, clim, m0, m1, _ = cases.make_case("conv_sedi", n=10)
    atm = synthetic_particles(n, seed=11, quantities=names)
    atm["q"][:] = 0.0
    for k, name in enumerate(names):
        if name == "m":
            atm["q"][k] = 1e7 * (1.0 + atm["lat"] / 180.0)
        elif name not in ACT:
            atm["q"][k] = 0.25 + np.cos(np.radians(atm["lon"]))
    _fill(atm, names)
    i = np.arange(n)
    ctl = dict(cases.BASE, **ctl_from_quantities(names))
    if direction == 1:
        atm["time"][:] = 60.0 * (i % 40) + 7.0 * (i % 3)
        atm["time"][::5] = 3000.0
        t = 2520.0
    else:
        ctl.update(direction=-1, t_stop=0.0)
        atm["time"][:] = 3600.0 - 60.0 * (i % 40) - 7.0 * (i % 3)
        atm["time"][::5] = 600.0
        t = 1080.0
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    s.set_radio_decay(names)
    s.timesteps_init(atm["time"].min(), atm["time"].max())
    s.module("timesteps", t)
    for _ in range(steps):
        s.module("radio_decay", t)
    g = s.state()
    dt = s.get_cache()["dt"]
    s.close()
    ref = atm["q"].copy()
    for _ in range(steps):
        refradio.apply(ref, _idx(names), dt, mode)
    return g, ref, dt, atm


SETS = [(a,) for a in ACT] + [ACT, ("m",) + ACT + ("vmr", "loss_rate"), ("Apb210", "m", "Arn222")]


@pytest.mark.parametrize("steps", [1, 20])
@pytest.mark.parametrize("names", SETS, ids=["+".join(x) for x in SETS])
def test_module_alone_against_restatement(names, steps):
    g, ref, dt, atm = single(names, steps=steps)
    moved = dt != 0
    assert (~moved).sum() > 10000 and moved.sum() > 50000 and np.all(dt[moved] > 0)
    assert np.array_equal(g["q"][:, ~moved], atm["q"][:, ~moved])                 # dt == 0: not touched
    for k, name in enumerate(names):
        if name in ACT:
            assert rel(g["q"][k], ref[k]) <= 1e-12, name
            assert np.all(g["q"][k][moved] != atm["q"][k][moved]), name            # the module acted
        else:                                                                      # m, vmr, loss_rate: unchanged
            assert np.array_equal(g["q"][k], atm["q"][k]), name
    if "Apb210" in names and "Arn222" in names:      # ingrowth: more Pb-210 than its own decay leaves
        k = names.index("Apb210")
        assert np.mean(g["q"][k][moved] > atm["q"][k][moved]) > 0.9
    for k in ("time", "p", "lon", "lat"):
        assert np.array_equal(g[k], atm[k]), k


def test_backward_in_time():
    """DIRECTION -1: negative dt, the same formula (the activities grow)"""
    g, ref, dt, atm = single(("m",) + ACT, direction=-1)
    moved = dt != 0
    assert (~moved).sum() > 10000 and np.all(dt[moved] < 0)
    assert np.array_equal(g["q"][:, ~moved], atm["q"][:, ~moved])
    assert np.array_equal(g["q"][0], atm["q"][0])
    for k in range(1, 7):
        assert rel(g["q"][k], ref[k]) <= 1e-12, ACT[k - 1]
    assert np.all(g["q"][1][moved] > atm["q"][1][moved])


def test_off_or_without_activities_nothing_happens():
    names = ("m",) + ACT
    ctl, clim, m0, m1, atm = cases.make_case("conv_sedi", n=2000, quantities=names)
    _fill(atm, names)
    for reg in (dict(quantities=names, on=False), dict(quantities=("m",), on=True), None):
        s = hip.Simulation(ctl, clim, m0, m1, atm)
        if reg is not None:
            s.set_radio_decay(**reg)
        s.timesteps_init(0.0, 0.0)
        s.run_timestep(0.0)
        s.run_timestep(180.0)
        g = s.state()
        s.close()
        assert np.array_equal(g["q"][1:], atm["q"][1:]), reg
    # ... but module_radio_decay on its own runs with the registration whether the step's switch is on or not
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    s.set_radio_decay(names, on=False)
    s.timesteps_init(0.0, 0.0)
    s.module("timesteps", 180.0)
    s.module("radio_decay", 180.0)
    g, dt = s.state(), s.get_cache()["dt"]
    s.close()
    assert rel(g["q"], refradio.apply(atm["q"].copy(), _idx(names), dt)) <= 1e-12


def test_refusals():
    names = ("m", "vmr", "loss_rate", "mloss_decay", "mloss_wet", "mloss_dry", "mloss_oh", "aoa", "Cccl4", "Csf6", "Cx",
             "Arn222", "Apb210")
    ctl, clim, m0, m1, atm = cases.make_case("conv_sedi", n=100, quantities=names)
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    good = _idx(names)
    s.set_radio_decay(good)

    def refused(idx, msg):
        with pytest.raises(hip.MphipError, match=msg):
            s.set_radio_decay(idx)
    refused([len(names)] + good[1:], r"outside \[0, nq")
    refused([11, 11, -1, -1, -1, -1], "is also activity Arn222")
    for k, taken in enumerate(names[:11]):
        refused([11, -1, k, -1, -1, -1], f"activity Abe7 \\(quantity {k}\\) is already quantity {taken}")
    # mphip_update_ctl keeps the registration valid
    s.ctl.qnt_aoa = 12
    with pytest.raises(hip.MphipError, match="activity Apb210 .* is already quantity aoa"):
        s.update_ctl()
    s.ctl.qnt_aoa = 7
    s.update_ctl()
    s.set_radio_decay([-1] * 6, on=False)
    s.ctl.qnt_aoa = 12            # (nothing registered: anything goes)
    s.update_ctl()
    s.close()


STEP_NAMES = ("m", "rp", "rhop") + ACT


def _stepping(n=4000, steps=20, multi=None, on=True, case="conv_sedi", **kw):
    ctl, clim, m0, m1, atm = cases.make_case(case, n=n, quantities=STEP_NAMES)
    _fill(atm, STEP_NAMES)
    ctl.update(kw)
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    s.set_radio_decay(STEP_NAMES, on=on)
    s.timesteps_init(atm["time"].min(), atm["time"].max())
    times = cases.step_times(s.ctl)[:steps]
    out = []
    if multi is not None:
        s.set_option("multi_step", multi)
        s.run_timestep(times[0])
        s.run_timesteps(times[1], len(times) - 1)
        out.append((times[-1], s.state(), s.get_cache()))
    else:
        for t in times:
            s.run_timestep(t)
            out.append((t, s.state(), s.get_cache()))
    s.close()
    return ctl, clim, m0, m1, atm, out


@pytest.mark.parametrize("case,kw", [("conv_sedi", {}),
                                     ("conv_sedi", dict(tdec_trop=259200.0, tdec_strat=259200.0, dry_depo_vdep=0.15,
                                                        wet_depo_ic_a=1e-4, wet_depo_ic_b=0.8, wet_depo_bc_a=5e-5,
                                                        wet_depo_bc_b=0.6))],
                         ids=["movers", "with_decay_and_deposition"])
def test_multi_step_launches_equal_single_steps(case, kw):
    *_, a = _stepping(multi=64, case=case, **kw)
    *_, b = _stepping(multi=0, case=case, **kw)
    ga, gb = a[-1][1], b[-1][1]
    assert a[-1][2]["rng_ctr"] == b[-1][2]["rng_ctr"]
    for k in ("time", "p", "lon", "lat", "q", "uvwp"):
        assert np.array_equal(ga[k], gb[k]), k


def test_twenty_steps_against_the_oracle():
    """conv_sedi (no module behind radio decay's place touches an activity): the oracle's time step and the restatement
    on its dt, step by step; with and without the module the particles move the same"""
    ctl, clim, m0, m1, atm, on = _stepping()
    *_, off = _stepping(on=False)
    o = B.Oracle(ctl, clim, m0, m1, atm)
    o.timesteps_init()
    idx = _idx(STEP_NAMES)
    for (t, g, cg), (_, h, ch) in zip(on, off):
        o.run_timestep(t)
        refradio.apply(o.q, idx, o.dt)
        for k in ("time", "p", "lon", "lat", "uvwp"):
            assert np.array_equal(g[k], h[k]), (t, k)
        assert np.array_equal(g["q"][:3], h["q"][:3]), t
        assert cg["rng_ctr"] == ch["rng_ctr"]
    assert len(on) == 20
    g, r = on[-1][1], o.state()
    assert np.array_equal(g["time"], r["time"])
    for k in ("lon", "lat", "p"):
        assert cases.rel_err(g[k], r[k]) <= 1e-10, k
    for k, name in enumerate(STEP_NAMES):
        assert rel(g["q"][k], r["q"][k]) <= 1e-10, name
        if name in ACT:
            assert not np.array_equal(g["q"][k], atm["q"][k]), name


def test_place_in_the_step():
    """C5's module set (module_sort, module_mixing, decay, wet and dry deposition, the movers) with the OH chemistry, the
    tracer chemistry and the six activities.  The activities against an oracle that carries them in its five trace-gas
    slots and the age-of-air slot (module_mixing mixes each quantity on its own) with the restatement behind the mixing;
    everything else against the same run with module_radio_decay off, bit for bit"""
    names = ("m", "vmr", "loss_rate", "mloss_oh") + TC.SPECIES + ("Csf6",) + ACT      # (15 of at most 16; no sedi)
    ctl, clim, m0, m1, atm = cases.make_case("full", n=4000, quantities=names, fields=TC.WITH_O3C)
    atm["q"][names.index("m")] *= 1e7
    atm["p"][::2] = 2.0 + 60.0 * np.random.default_rng(3).uniform(size=atm["p"][::2].size)
    TC._fill_tracers(atm, names)
    _fill(atm, names)
    for k in (names.index(x) for x in ACT):          # gradients for the mixing to act on
        atm["q"][k] *= 1.0 + 0.5 * np.cos(np.radians(atm["lat"]))
    ctl.update(oh_chem_reaction=3, oh_chem=TC.SO2_OH, tracer_chem=1)
    dclim, oclim = TC._clims(clim, extra={"oh": TC.OH})
    runs = {}
    for on in (True, False):
        s = hip.Simulation(ctl, dclim, m0, m1, atm)
        s.set_radio_decay(names, on=on)
        s.timesteps_init(atm["time"].min(), atm["time"].max())
        times = cases.step_times(s.ctl)
        for t in times:
            s.run_timestep(t)
        runs[on] = s.state()
        s.close()
    # the activities' oracle: the same particles and movers; trace gases and age of air are the activities
    act = [names.index(x) for x in ACT]
    octl = dict(ctl, qnt_tracer=tuple(act[:5]), qnt_aoa=act[5], tracer_chem=0)
    o = B.Oracle(octl, oclim, m0, m1, atm)
    o.timesteps_init()
    c = o.ctl
    mixed = 0
    for t in times:
        o.module("timesteps", t)
        if c.sort_dt > 0 and np.fmod(t, c.sort_dt) == 0:
            o.sort()
        for m in ("position", "advect", "diff_turb", "diff_meso", "convection", "position"):
            o.module(m)
        if np.fmod(t, c.mixing_dt) == 0:
            o.module("mixing", t)
            mixed += 1
        refradio.apply(o.q, act, o.dt)
    assert mixed >= 3 and len(times) >= 20
    g, h, r = runs[True], runs[False], o.state()
    for k in ("time", "lon", "lat", "p"):
        assert np.array_equal(g[k], h[k]), k
    for k, name in enumerate(names):
        if name not in ACT:
            assert np.array_equal(g["q"][k], h["q"][k]), name
    assert np.array_equal(g["time"], r["time"])
    for k in ("lon", "lat", "p"):
        assert cases.rel_err(g[k], r[k]) <= 1e-10, k
    for k in act:
        assert rel(g["q"][k], r["q"][k]) <= 1e-10, names[k]
        assert not np.array_equal(g["q"][k], h["q"][k]), names[k]      # (the module acted; off: mixed only)
        assert not np.array_equal(h["q"][k], atm["q"][k]), names[k]    # (mixing acts on them with the module off too)


def test_two_shards_with_mixing_give_the_single_context():
    """positions bit for bit; the activities to 1e-13 (the mixing's cell sums: two partial sums instead of one serial
    sum, as tests/test_gpu_full_size.py has it for the other mixed quantities)"""
    world, n = 2, 40000
    names = ("m", "vmr") + ACT
    ctl, clim, m0, m1, atm = cases.make_case("full", n=n, quantities=names)
    ctl.update(sort_dt=-999.0, mixing_dt=180.0)
    _fill(atm, names)
    one = hip.Simulation(ctl, clim, m0, m1, atm)
    one.set_radio_decay(names)
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
            s.set_radio_decay(names)
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
    for k in ("time", "lon", "lat", "p"):
        assert np.array_equal(np.concatenate([g[k] for _, _, g in out]), ref[k]), k
    q = np.concatenate([g["q"] for _, _, g in out], axis=1)
    for k in range(2, 2 + len(ACT)):
        assert rel(q[k], ref["q"][k]) <= 1e-13, names[k]
        assert not np.array_equal(ref["q"][k], atm["q"][k]), names[k]


def test_c3_at_1e7_against_the_restatement_on_a_sample():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import gpu_radio_decay_cost as cost
    n, n_steps = 10 ** 7, 10
    ctl, clim, met0, met1, atm, idx = cost.radio_inputs("on", n_steps + 1, n)
    s = hip.Simulation(ctl, clim, met0, met1, atm)
    s.set_radio_decay(idx)
    s.timesteps_init(0.0, 0.0)
    dt = s.ctl.dt_mod
    s.run_timestep(0.0)
    s.run_timesteps(dt, n_steps - 1)
    g = s.state()
    s.close()
    # (C3: every particle takes every step with dt = DT_MOD, but the first one at t = T_START, where dt = 0)
    assert np.all(g["time"] == (n_steps - 1) * dt)
    pick = np.random.default_rng(20261016).choice(n, 20000, replace=False)
    ref = atm["q"][:, pick].copy()
    for _ in range(n_steps - 1):
        refradio.apply(ref, idx, np.full(len(pick), dt))
    for j, k in enumerate(idx):
        assert rel(g["q"][k][pick], ref[k]) <= 1e-12, ACT[j]
    assert np.array_equal(g["q"][:3], atm["q"][:3])   # m, rp, rhop
