"""The axis searches of the device code on the inputs where their first guesses fail (tests/axis_cases.py): uneven
latitudes in either direction, a pressure axis with several nodes per bin of the pressure table in either direction,
particles on every grid line, one ulp beside it, on and beyond the ends of the axes.

The lean kernels (specialised step_kernel instantiations, depo_kernel, sort_key_kernel<true>, traj_tile_kernel) check a
guessed stencil once (lon_fast, lat_fast, p_fast, raw_cell_fast) and send a failing lane through the general code;
the general code corrects its own guesses (lat_guess / p_guess, locate_from).  Reference: the CPU oracle, which
tests/test_axis_edges_cpu.py holds against the numpy restatement on the same inputs.  Bars are the project's own
(tests/test_gpu_parity.py:_compare): positions and quantity rows within 1e-10, time, cache->uvwp and the counter of
the random numbers equal, sort keys and permutations equal.

Every test prints what it measured (one "AXIS_EDGE {json}" line per comparison) before it asserts.
tests/test_gpu_axis_edges_exact.py repeats the single modules and a run in the reference-rounding build with
tolerance 0, through the functions of this file."""
import functools
import json

import numpy as np
import pytest

import axis_cases as A
import cases
from mptrac_amd import hip
from oracle import binding as B

pytestmark = pytest.mark.gpu

TOL = 1e-10          # north_star tolerance for positions / quantities
SMALL = A.GRIDS[0]
# (grid, lon0, latitude axis, pressure axis): every warp on the small grid, both full warps on the one-degree grid
COMBOS = [(g, lon0, lat, p) for g in A.GRIDS for lon0 in A.LON0 for lat, p in (A.WARPS if g != "C1" else A.WARPS[:2])]


def _id(combo):
    g, lon0, lat, p = combo
    return "%s-lon%d-%s-%s" % (g if isinstance(g, str) else "x".join(map(str, g)), lon0, lat, p)


combos = pytest.mark.parametrize("combo", COMBOS, ids=_id)      # (closest to the function: inputs of a grid are reused)


@functools.lru_cache(maxsize=2)
def _inputs(case, combo):
    """(ctl, clim, met0, met1, atm, placed); the preconditions on the inputs are asserted in axis_cases.setup"""
    grid, lon0, lat, p = combo
    ctl, clim, m0, m1, atm, placed = A.setup(case, grid, lon0, lat, p, n=4096 if grid == "C1" else 2048)
    for name_q in ("zeta", "eta"):          # (make_case derives them from the latitude: keep them inside the zetal field)
        row = ctl.get("qnt_" + name_q, -1)
        if row >= 0:
            atm["q"][row] = 320.0 + 1680.0 * ((np.clip(atm["lat"], -85.0, 85.0) + 85.0) / 170.0)
    return ctl, clim, m0, m1, atm, placed


def _pair(case, combo, over=None, options=None):
    ctl, clim, m0, m1, atm, _ = _inputs(case, combo)
    ctl = dict(ctl, **(over or {}))
    o = B.Oracle(ctl, clim, m0, m1, atm)
    o.timesteps_init()
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    for k, v in (options or {}).items():
        s.set_option(k, v)
    s.timesteps_init(atm["time"].min(), atm["time"].max())
    assert s.ctl.t_start == o.ctl.t_start and s.ctl.t_stop == o.ctl.t_stop
    return o, s, atm


def errors(o, s):
    g, r = s.state(), o.state()
    e = {k: cases.rel_err(g[k], r[k]) for k in ("lon", "lat", "p")}
    e["q"] = cases.q_rows_err(o.ctl, g["q"], r["q"])[0] if r["q"].size else 0.0
    e["time"] = bool(np.array_equal(g["time"], r["time"]))
    e["uvwp"] = bool(np.array_equal(g["uvwp"], r["uvwp"]))
    e["ctr"] = bool(s.get_cache()["rng_ctr"] == o.cache.rng_ctr)
    return e


def check(e, tol, **tag):
    """tol = 0: array_equal (rel_err and q_rows_err are 0 only for equal arrays with equal NaN patterns)"""
    print("AXIS_EDGE " + json.dumps(dict(tag, **e)))
    assert e["time"] and e["uvwp"] and e["ctr"], (tag, e)
    for k in ("lon", "lat", "p", "q"):
        assert e[k] <= tol, (tag, k, e[k])


# ---------------------------------------------------------------------------
# one module at a time, from the exact positions
# ---------------------------------------------------------------------------

# "movers": module_diff_turb, module_diff_meso, module_convection, module_sedi and module_position as ONE call of the C
# ABI (a module mask) -- the lean instantiation for the movers behind module_advect, the only lean step kernel that meets
# the exact positions before module_position has touched them (on an ascending pressure axis that matters: see RUNS)
MOVERS = ("diff_turb", "diff_meso", "convection", "sedi")
GROUPS = {"conv_sedi": ["advect4", "advect2", "advect1", "diff_turb", "diff_meso", "convection", "sedi", "movers"],
          "meteo": ["meteo"],
          "full": ["wet_depo", "dry_depo"]}


def single_modules(case, combo, tol=TOL):
    """Every module of the group from the same positions: a step moves a particle off its grid line, so the particle set
    is uploaded again before each module; module_timesteps first (the second call of the time loop: dt = DT_MOD).
    The single-module calls run the general code: lat_guess / p_guess, locate_from, locate_lon / locate_reg."""
    o, s, atm = _pair(case, combo)
    t = cases.step_times(o.ctl)[1]
    start = {k: np.array(atm[k], dtype=np.float64) for k in ("time", "lon", "lat", "p", "q")}
    moved = {}
    for name in GROUPS[case]:
        for k in ("time", "lon", "lat", "p"):
            getattr(o, k)[:] = start[k]
        o.q[:] = start["q"].reshape(o.q.shape)
        s.update_atm(atm)
        module = name
        if name.startswith("advect"):
            module, o.ctl.advect, s.ctl.advect = "advect", int(name[6:]), int(name[6:])
            s.update_ctl()
        for eng in (o, s):
            eng.module("timesteps", t)
        assert np.array_equal(s.get_cache()["dt"], o.dt) and np.count_nonzero(o.dt) == o.n
        if name == "movers":
            for m in MOVERS + ("position",):
                o.module(m, t)
            s._chk(s.L.mphip_module(s.h, sum(hip.MOD[m] for m in ("timesteps",) + MOVERS + ("position2",)), t))
        else:
            o.module(module, t)
            s.module(module, t)
        check(errors(o, s), tol, test="single", case=case, combo=_id(combo), module=name)
        r = o.state()
        moved[name] = int(np.count_nonzero((r["lon"] != start["lon"]) | (r["lat"] != start["lat"]) | (r["p"] != start["p"])
                                           | np.any(r["q"] != start["q"].reshape(r["q"].shape), axis=0)))
        assert moved[name] >= 10, (name, moved[name])      # (the module acted; dry deposition: the surface layer only)
    s.close()
    return moved


@pytest.mark.parametrize("case", list(GROUPS))
@combos
def test_single_modules_at_the_exact_positions(combo, case):
    single_modules(case, combo)


# ---------------------------------------------------------------------------
# module_sort: keys and permutation
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("interval", [0, 1])
@combos
def test_sort_keys_and_permutation(combo, interval):
    """sort_key_kernel<true> through raw_cell_fast -- the product with the reciprocal spacing decides the longitude
    index unless it lands within 1e-9 of a whole number, which is where every on-node particle lands -- against
    module_sort of the oracle: keys, permutation (ties by index: the on-node triples share their boxes) and permuted
    arrays; once on the exact positions, and once after two steps from the device's state."""
    o, s, atm = _pair("full", combo, options={"locality_sort_interval": interval})
    _, _, m0, _, _, placed = _inputs("full", combo)
    for round_ in (0, 1):
        keys_o, perm_o = o.sort()
        keys_s, perm_s = s.sort()
        same = bool(np.array_equal(np.sort(keys_o), keys_s)) and bool(np.array_equal(perm_o, perm_s))
        print("AXIS_EDGE " + json.dumps(dict(test="sort", combo=_id(combo), interval=interval, round=round_, equal=same,
                                             differing=int(np.count_nonzero(perm_o != perm_s)))))
        assert np.array_equal(np.sort(keys_o), keys_s)      # device returns the sorted keys
        assert np.array_equal(perm_o, perm_s)
        g, r = s.state(), o.state()
        for k in ("time", "lon", "lat", "p", "q"):
            assert np.array_equal(g[k], r[k]), k
        if round_ == 0:
            assert len(np.unique(keys_o[:placed])) <= placed - 48      # (ties among the on-node particles)
            for t in cases.step_times(o.ctl)[:3]:
                s.run_timestep(t)
            g = s.state()
            for k in ("time", "p", "lon", "lat"):       # both sides continue from the same bits (the device's)
                getattr(o, k)[:] = g[k]
            o.q[:] = g["q"]
    s.close()


# ---------------------------------------------------------------------------
# lean instantiations against the general code
# ---------------------------------------------------------------------------

LEAN_SETS = {"c3_set": dict(),
             "c3_set_decay_deposition": dict(tdec_trop=259200.0, tdec_strat=259200.0, dry_depo_vdep=0.15, wet_depo_ic_a=1e-4,
                                             wet_depo_ic_b=0.8, wet_depo_bc_a=5e-5, wet_depo_bc_b=0.6)}


@pytest.mark.parametrize("advect", [4, 2, 1], ids=["rk4", "midpoint", "euler"])
@pytest.mark.parametrize("modules", list(LEAN_SETS))
@combos
def test_lean_instantiations_equal_the_general_code(combo, modules, advect):
    """Options of test_gpu_parity.py:test_lean_instantiations_equal_the_general_code on the warped grids: the first
    stage of the first moving step sets up its stencil on the exact positions, where the checked guess of a lean
    kernel fails and the lane recomputes with the general code -- same bits as the general kernel in every array."""
    ctl, clim, m0, m1, atm, _ = _inputs("conv_sedi", combo)
    ctl = dict(ctl, advect=advect, **LEAN_SETS[modules])
    runs = []
    for generic in (0, 1):
        s = hip.Simulation(ctl, clim, m0, m1, atm)
        s.set_option("generic_kernel", generic)
        s.timesteps_init(0.0, 0.0)
        for t in cases.step_times(s.ctl)[:6]:
            s.run_timestep(t)
        runs.append(s.state())
        s.close()
    diff = {k: int(np.count_nonzero(~((runs[0][k] == runs[1][k]) | (np.isnan(runs[0][k]) & np.isnan(runs[1][k])))))
            for k in ("time", "lon", "lat", "p", "q", "uvwp")}
    print("AXIS_EDGE " + json.dumps(dict(test="lean", combo=_id(combo), modules=modules, advect=advect, differing=diff)))
    for k in ("time", "lon", "lat", "p", "q", "uvwp"):
        assert np.array_equal(runs[0][k], runs[1][k]), (k, diff)
    assert np.count_nonzero(runs[0]["lon"] != atm["lon"]) > len(atm["lon"]) // 2


# ---------------------------------------------------------------------------
# whole runs
# ---------------------------------------------------------------------------

# On an ascending pressure axis module_position and module_diff_turb of the reference take met->p[np - 1] for the top of
# the model, which is then the surface node: module_position reflects every particle to a pressure beyond that node
# (p_top^2 / p) in the first moving step, and the vertical turbulent step clamps to it.  Oracle and device follow the
# reference in this, so the whole steps are compared all the same, but from then on they search beyond the end of the
# axis only.  Inside an ascending axis the searches are covered by the single modules and the "movers" launch above, by
# module_sort and the deposition kernels, and by the module sequence without module_position below.
RUNS = [(SMALL, -180.0, "uneven", "crowded"), ("C1", 0.0, "uneven", "crowded"),
        (SMALL, 0.0, "reversed_uneven", "crowded_ascending"), ("C1", -180.0, "reversed_uneven", "crowded_ascending")]


def whole_run(case, combo, tol=TOL, nsteps=20, modes=("steps", "batched")):
    ctl, clim, m0, m1, atm, _ = _inputs(case, combo)
    o = B.Oracle(ctl, clim, m0, m1, atm)
    o.timesteps_init()
    times = cases.step_times(o.ctl)[:nsteps]
    for t in times:
        o.run_timestep(t)
    for k in ("lon", "lat", "p"):
        assert np.all(np.isfinite(getattr(o, k))), k
    for mode in modes:
        s = hip.Simulation(ctl, clim, m0, m1, atm)
        s.timesteps_init(atm["time"].min(), atm["time"].max())
        if mode == "steps":
            for t in times:
                s.run_timestep(t)
        else:                              # the multi-step instantiations: steps that share a launch
            s.run_timestep(times[0])
            s.run_timesteps(times[1], len(times) - 1)
        check(errors(o, s), tol, test="run", case=case, combo=_id(combo), mode=mode, steps=len(times))
        s.close()


@pytest.mark.parametrize("case", ["conv_sedi", "full"])
@pytest.mark.parametrize("combo", RUNS, ids=_id)
def test_twenty_steps_against_the_oracle(combo, case):
    whole_run(case, combo)


@pytest.mark.parametrize("combo", [c for c in RUNS if c[3] == "crowded_ascending"], ids=_id)
def test_twenty_steps_without_module_position_on_an_ascending_axis(combo):
    """The oracle cannot keep particles inside an ascending pressure axis through whole steps (module_position, see
    RUNS), so this variant is the module sequence advection, horizontal turbulent and mesoscale diffusion, module_meteo:
    20 steps, module by module on both sides."""
    o, s, atm = _pair("meteo", combo, over=dict(turb_dz_trop=0.0, turb_dz_strat=0.0, turb_dz_pbl=0.0))
    p_lo, p_hi = float(o._mets[0].p.min()), float(o._mets[0].p.max())
    for t in cases.step_times(o.ctl)[:20]:
        for m in ("timesteps", "advect", "diff_turb", "diff_meso"):
            o.module(m, t)
            s.module(m, t)
    o.module("meteo")
    s.module("meteo")
    inside = float(np.mean((o.p > p_lo) & (o.p < p_hi)))
    assert inside > 0.9, inside               # (the particles are still inside the axis)
    check(errors(o, s), TOL, test="sequence", combo=_id(combo), inside=inside)
    s.close()


# ---------------------------------------------------------------------------
# LDS tile trajectories
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("advect", [4, 2, 1], ids=["rk4", "midpoint", "euler"])
@pytest.mark.parametrize("tile", [1024, 96])
@pytest.mark.parametrize("combo", [("C1", -180.0, "uneven", "crowded"), (SMALL, 0.0, "reversed_uneven", "crowded_ascending")], ids=_id)
def test_lds_tile_trajectories_equal_the_launches_without_a_tile(combo, tile, advect):
    """Options of test_gpu_parity.py:test_lds_tile_trajectories_equal_the_launches_without_a_tile on a warped grid:
    traj_tile_kernel's stencils from the checked guesses, same bits with and without the tile, and the oracle's positions."""
    grid, lon0, lat, p = combo
    ctl, clim, m0, m1, atm, _ = A.setup("advect", grid, lon0, lat, p, n=4096, over=dict(advect=advect),
                                        fields=("u", "v", "w", "ps"), quantities=("m",))
    atm["time"][::11] = 540.0
    o = B.Oracle(ctl, clim, m0, m1, atm)
    o.timesteps_init()
    times = cases.step_times(o.ctl)[:14]
    runs = []
    for cells in (0, tile):
        s = hip.Simulation(ctl, clim, m0, m1, atm)
        s.set_option("lds_tile", cells)
        s.set_option("locality_sort_interval", 5)
        s.timesteps_init(atm["time"].min(), atm["time"].max())
        s.run_timestep(times[0])
        s.synchronize()
        s.profile_begin()
        s.run_timesteps(times[1], 4)
        launches, _ = s.profile_end()
        assert launches == 1
        s.run_timesteps(times[5], 9)
        runs.append(s.state())
        s.close()
    for k in ("time", "lon", "lat", "p", "q"):
        assert np.array_equal(runs[0][k], runs[1][k]), k
    for t in times:
        o.run_timestep(t)
    r = o.state()
    e = {k: cases.rel_err(runs[1][k], r[k]) for k in ("lon", "lat", "p")}
    print("AXIS_EDGE " + json.dumps(dict(test="tile", combo=_id(combo), tile=tile, advect=advect, **e)))
    assert np.array_equal(runs[1]["time"], r["time"])
    for k in ("lon", "lat", "p"):
        assert e[k] <= TOL, (k, e[k])


# ---------------------------------------------------------------------------
# winds from the model levels
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["zeta_full", "mlp_full"])
@pytest.mark.parametrize("combo", [(SMALL, -180.0, "uneven", "ladder"), ("C1", 0.0, "uneven", "ladder")], ids=_id)
def test_model_levels_on_uneven_latitudes(combo, case):
    """The lean model-level instantiations take longitude and latitude indices from the checked guesses (the `guessed`
    branch beside locate_pairs4): on-node longitudes and latitudes on the uneven latitude axis, 8 steps."""
    whole_run(case, combo, nsteps=8)
