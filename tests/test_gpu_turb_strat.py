"""module_diff_turb's short path above every tropopause (diff_turb_fast, DevMet::strat_skip, option turb_strat): a wave
whose lanes all pass `far && 1.01 p < strat_skip && |lat| <= 90` leaves out the tropopause look-up, the weights, the
blends and the first Box-Muller pair.  The path must not be observable: every case runs the lean kernel with turb_strat
1 against turb_strat 0 and against the general kernel (option generic_kernel 1), array_equal on time, lon, lat, p, every
quantity and uvwp -- as one launch per step and as one mphip_run_timesteps call of five steps, forward and backward.
The reference-rounding build is compared with the oracle's bits in a child process (a process loads one library).

Grid C1, C3's module set (advection, turbulent and mesoscale diffusion, convection, sedimentation) with turb_dz_trop
0.5 next to turb_dz_strat 0.1, so that a tropopause weight that is not 0 shows in the bits.  Particles: `strat` ones
uniform in 18.5 ... 29.5 km (the bound is 84.6 hPa / 1.01: 17.45 km), the rest hand-placed per case (CASES below).

Break checks, each tried once on a scratch copy of the sources (profiles/r09_turb_strat_ab.txt lists the failing tests):
a wrong Kz in the short path, the latitude clause dropped, the surface re-do dropped.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import turbstrat as TS
from mptrac_amd import hip
from mptrac_amd.clim import load_clim_tropo
from mptrac_amd.synth import Met, pressure_from_z, synthetic_met, synthetic_particles

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STATE = ("time", "lon", "lat", "p", "q", "uvwp")
STEPS = 5
DAY = 86400.0
CLIM = load_clim_tropo()
BOUND = TS.strat_bound(CLIM)      # (the steep-pole table of case c has the same: its pole nodes are the table's minimum)
P_BOUND = BOUND / 1.01            # the device's test is 1.01 p < bound
BASE = dict(cases.CASES["conv_sedi"], turb_dz_trop=0.5)


@functools.lru_cache(maxsize=None)
def _base_mets():
    f = cases.PRESSURE_LEVEL_FIELDS
    return synthetic_met("C1", 0.0, 1.0, fields=f), synthetic_met("C1", 3600.0, 1.25, fields=f)


@functools.lru_cache(maxsize=None)
def _mets(kind, t0):
    """the two snapshots at t0 and t0 + 3600 s (the fields are shared, never written).  polar: 20 m/s towards the pole in
    the two rows next to each pole, 0.03 degrees per step; regional: the longitude axis 10 ... 370 degrees -- it does not
    start in [-360, 0], so every shortcut bound of DevMet is off"""
    out = []
    for k, m in enumerate(_base_mets()):
        f3, lon = m.f3, m.lon
        if kind == "polar":
            v = m.f3["v"].copy()
            v[:, -2:, :], v[:, :2, :] = 20.0, -20.0
            f3 = dict(m.f3, v=v)
        if kind == "regional":
            lon = m.lon + 190.0
        out.append(Met(t0 + 3600.0 * k, lon, m.lat, m.p, f3, m.f2))
    return tuple(out)


def _strat(n, seed=4711):
    return synthetic_particles(n, seed=seed, quantities=cases.QUANTITIES, z=(18.5, 29.5))


def _put(atm, i, **kw):
    for k, v in kw.items():
        atm[k][i] = v
    return atm


def _mixed(n):
    """64 particles above the bound and n - 64 over the whole depth"""
    a, b = _strat(64), synthetic_particles(n - 64, seed=99, quantities=cases.QUANTITIES)
    return {k: np.ascontiguousarray(np.concatenate([a[k], b[k]], axis=-1)) for k in a}


def _polar(atm):
    # 1.01 p inside (edge of the steep table at 90.02 degrees, bound) = (81.2, 84.6) hPa: tropopause weight 0.06 there
    _put(atm, 7, lon=45.0, lat=89.99, p=0.99 * P_BOUND)
    _put(atm, 9, lon=-120.0, lat=-89.99, p=0.99 * P_BOUND)
    return atm


# name: (particles, control settings on top of BASE, snapshots, start of the hour, climatology)
CASES = {
    # (a) waves entirely above the bound
    "a_64": (lambda: _strat(64), {}, "plain", 0.0, CLIM),
    "a_65": (lambda: _strat(65), {}, "plain", 0.0, CLIM),
    "a_257": (lambda: _strat(257), {}, "plain", 0.0, CLIM),
    # (b) one lane of the wave beside the bound
    "b_just_below": (lambda: _put(_strat(64), 17, p=P_BOUND * (1.0 - 1e-6)), {}, "plain", 0.0, CLIM),
    "b_just_above": (lambda: _put(_strat(64), 17, p=P_BOUND * (1.0 + 1e-6)), {}, "plain", 0.0, CLIM),
    "b_at": (lambda: _put(_strat(64), 17, p=P_BOUND), {}, "plain", 0.0, CLIM),
    "b_ulp_below": (lambda: _put(_strat(64), 17, p=np.nextafter(P_BOUND, 0.0)), {}, "plain", 0.0, CLIM),
    "b_ulp_above": (lambda: _put(_strat(64), 17, p=np.nextafter(P_BOUND, np.inf)), {}, "plain", 0.0, CLIM),
    # (c) two lanes that the advection takes across a pole, on the table whose end cells are steep
    "c_pole": (lambda: _polar(_strat(64)), {}, "polar", 0.0, TS.steep_pole_clim(CLIM)),
    # (d) a NaN pressure; a pressure above the top of the axis (0.19 hPa)
    "d_nan": (lambda: _put(_strat(64), 23, p=np.nan), {}, "plain", 0.0, CLIM),
    "d_above_top": (lambda: _put(_put(_strat(64), 23, p=0.1), 40, p=0.19), {}, "plain", 0.0, CLIM),
    # (e) the stratosphere's parameters
    "e_dx_strat": (lambda: _mixed(128), dict(turb_dx_strat=50.0), "plain", 0.0, CLIM),
    "e_dz_strat_0": (lambda: _mixed(128), dict(turb_dz_strat=0.0), "plain", 0.0, CLIM),
    # a drift of -257 km and sigma_z 60 km per step (dz2dp is linear in dz: p grows 38 +- 9 fold): most lanes pass the
    # boundary-layer bound in the first step, on the short path, and are reflected again at the interpolated surface
    "e_dz_strat_huge": (lambda: _strat(128), dict(turb_dz_strat=1e7), "plain", 0.0, CLIM),
    # (f) the first and the last fortnight of the year: the month axis (day 14 ... 349) is continued
    "f_day_5": (lambda: _mixed(128), {}, "plain", 5 * DAY, CLIM),
    "f_day_360": (lambda: _mixed(128), {}, "plain", 360 * DAY, CLIM),
    # (g) the bound off; the instantiations with the boundary-layer closure; the two-stage integrator
    "g_regional": (lambda: _put(_mixed(128), slice(None), lon=_mixed(128)["lon"] + 190.0), {}, "regional", 0.0, CLIM),
    "g_pbl_scheme": (lambda: _mixed(128), dict(turb_pbl_scheme=1, turb_mesoz=0.0), "plain", 0.0, CLIM),
    "g_midpoint": (lambda: _mixed(128), dict(advect=2), "plain", 0.0, CLIM),
}


def inputs(name, direction):
    make, over, kind, t0, clim = CASES[name]
    atm = make()
    ctl = dict(BASE, **cases.ctl_from_quantities(cases.QUANTITIES))
    ctl.update(over)
    if direction == 1:
        ctl.update(t_stop=t0 + 3600.0)
        atm["time"][:] = t0
    else:
        ctl.update(direction=-1, t_stop=t0)
        atm["time"][:] = t0 + 3600.0
    m0, m1 = _mets(kind, t0)
    return ctl, clim, m0, m1, atm


def run_device(inp, form, turb_strat=1, generic=0):
    ctl, clim, m0, m1, atm = inp
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    try:
        s.set_option("turb_strat", turb_strat)
        s.set_option("generic_kernel", generic)
        s.timesteps_init(float(atm["time"].min()), float(atm["time"].max()))
        times = cases.step_times(s.ctl)
        if form == "multi":
            s.run_timesteps(times[1], STEPS)
        else:
            for t in times[1:1 + STEPS]:
                s.run_timestep(t)
        return s.state(), s.shortcuts()
    finally:
        s.close()


def run_oracle(inp):
    from oracle import binding as B
    ctl, clim, m0, m1, atm = inp
    o = B.Oracle(ctl, clim, m0, m1, atm)
    o.timesteps_init()
    for t in cases.step_times(o.ctl)[1:1 + STEPS]:
        o.run_timestep(t)
    return o.state()


def differing(a, b):
    return {k: int(np.count_nonzero(~((a[k] == b[k]) | (np.isnan(a[k]) & np.isnan(b[k]))))) for k in STATE
            if not np.array_equal(a[k], b[k], equal_nan=True)}


@pytest.mark.parametrize("direction", [1, -1], ids=["forward", "backward"])
@pytest.mark.parametrize("form", ["single", "multi"])
@pytest.mark.parametrize("name", list(CASES))
def test_short_path_is_not_observable(name, form, direction):
    inp = inputs(name, direction)
    on, bounds = run_device(inp, form, turb_strat=1)
    off, _ = run_device(inp, form, turb_strat=0)
    general, _ = run_device(inp, "single", generic=1)
    assert not differing(on, off), ("turb_strat 1 / 0", differing(on, off))
    assert not differing(on, general), ("lean / general", differing(on, general))
    # the run did something: every particle with a pressure moved five steps, vertically too
    atm = inp[4]
    live = ~np.isnan(atm["p"])
    assert np.all(on["time"][live] == atm["time"][live] + direction * STEPS * BASE["dt_mod"])
    assert np.count_nonzero(on["p"][live] != atm["p"][live]) == live.sum()
    assert (bounds["turb"] == -np.inf) == (name == "g_regional")      # (turb_skip: the short path rests on it)


def test_the_cases_stand_where_they_are_meant_to():
    """the inputs against the restated bound: which particles pass the device's test at the start"""
    def passes(atm):
        with np.errstate(invalid="ignore"):
            return (atm["p"] * 1.01 < BOUND) & (np.abs(atm["lat"]) <= 90.0)
    for name in ("a_64", "a_65", "a_257", "b_just_below", "b_ulp_below", "c_pole", "d_above_top", "e_dz_strat_huge"):
        assert passes(CASES[name][0]()).all(), name
    for name in ("b_just_above", "b_at", "b_ulp_above", "d_nan"):
        ok = passes(CASES[name][0]())
        assert ok.sum() == 63 and not ok[17 if name.startswith("b") else 23], name
    assert P_BOUND * 1.01 >= BOUND > np.nextafter(P_BOUND, 0.0) * 1.01
    mixed = passes(_mixed(128))
    assert mixed[:64].all() and 10 < mixed[64:].sum() < 54
    assert pressure_from_z(17.4) > P_BOUND > pressure_from_z(17.5)
    # the polar lanes: one step of 20 m/s takes them 0.03 degrees, across the pole
    atm = CASES["c_pole"][0]()
    assert 90.0 - abs(atm["lat"][7]) < 20.0 * BASE["dt_mod"] / 111e3 and abs(atm["lat"][9]) == abs(atm["lat"][7])


CHILD = r"""
import json, sys
sys.path[:0] = [ROOT, ROOT + "/tests"]
from mptrac_amd import hip
import test_gpu_turb_strat as T
print("library:", hip.load().mphip_version().decode())
direction = int(sys.argv[1])
for name in sys.argv[2:]:
    inp = T.inputs(name, direction)
    ref = T.run_oracle(inp)
    row = dict(case=name)
    for form in ("single", "multi"):
        got, _ = T.run_device(inp, form)
        row[form] = T.differing(got, ref)
    print("TURBSTRAT " + json.dumps(row))
""".replace("ROOT", repr(ROOT))

_NAMES = list(CASES)
GROUPS = [_NAMES[0::3], _NAMES[1::3], _NAMES[2::3]]


@pytest.mark.parametrize("direction", [1, -1], ids=["forward", "backward"])
@pytest.mark.parametrize("names", GROUPS, ids=["cases_0", "cases_1", "cases_2"])
def test_reference_rounding_build_has_the_oracles_bits(names, direction):
    env = dict(os.environ, MPTRAC_AMD_EXACT="1")
    env.pop("MPHIP_LIB", None)
    res = subprocess.run([sys.executable, "-c", CHILD, str(direction), *names], capture_output=True, text=True, timeout=300,
                         env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-3000:]
    lib = [ln for ln in res.stdout.splitlines() if ln.startswith("library:")][0]
    assert "reference rounding" in lib, lib
    rows = [json.loads(ln[10:]) for ln in res.stdout.splitlines() if ln.startswith("TURBSTRAT ")]
    assert [r["case"] for r in rows] == names
    for r in rows:
        for k in ("single", "multi"):
            assert not r[k], (r["case"], k, r[k])
