"""The decisions of module_convection, module_wet_depo and module_dry_depo on the device at their edges
(tests/depo_cases.py): particles on a threshold and one ulp beside it, NaN and infinite surface fields and the
nearest-neighbour rules, every option set, and the four shortcuts that let a particle leave before it gathers anything
(DevMet::pct_skip, ps_skip, conv_skip, turb_skip) on their bounds, inside their guard bands, at and beside the snapshot
times and beyond the ends of the horizontal axes.

Reference: the CPU oracle, which tests/test_depo_edges_cpu.py holds against the numpy restatement on the same cases.
  - a particle the oracle leaves untouched is bit-untouched on the device, in p, lon, lat and every quantity;
  - a particle the oracle acts on is acted on by the device;
  - the values are within the suite's parity bar (tests/test_gpu_parity.py:_compare, 1e-10), and equal to the oracle's
    in the reference-rounding build (tests/test_gpu_depo_edges_exact.py runs this file's functions with tol = 0);
  - where the oracle's value is not finite (pct == pcb: dz = 0) the device's is of the same class (NaN, +inf, -inf);
  - every launch shape of one build gives the same bits.

Every comparison prints what it measured (one "DEPO_EDGE {json}" line) before it asserts."""
import functools
import json

import numpy as np
import pytest

import cases
import depo_cases as D
import refradiodepo as RD
from mptrac_amd import hip
from mptrac_amd.ctl import RADIO_ACTIVITIES
from oracle import binding as B
import test_depo_edges_cpu as CPU
from test_gpu_parity import TOL, _compare

pytestmark = pytest.mark.gpu

NAMES = sorted(D.all_cases())
FAMILIES = sorted({n.split("-")[0] for n in NAMES})
KEYS = ("time", "lon", "lat", "p", "q", "uvwp")


def _same(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _primed(engine, case):
    """module_timesteps at case["t"] with every particle on an interior node (outside a grid that is not periodic the
    module sets dt = 0, mptrac.c:6030-6035; a particle that left the domain within the step keeps its dt), then the
    case's positions."""
    engine.ctl.t_start, engine.ctl.t_stop = D.T_START, D.T_STOP
    if isinstance(engine, hip.Simulation):
        engine.update_ctl()
    engine.module("timesteps", case["t"])
    return engine


def pair(case, options=None):
    atm = case["atm"]
    inside = dict(atm, lon=np.full_like(atm["lon"], case["m0"].lon[1]), lat=np.full_like(atm["lat"], case["m0"].lat[1]))
    o = _primed(B.Oracle(case["ctl"], case["clim"], case["m0"], case["m1"], inside), case)
    s = hip.Simulation(case["ctl"], case["clim"], case["m0"], case["m1"], inside)
    for k, v in (options or {}).items():
        s.set_option(k, v)
    _primed(s, case)
    dt = s.get_cache()["dt"]
    assert np.array_equal(dt, o.dt) and np.array_equal(dt, case["t"] - atm["time"]) and np.all(dt != 0)
    for k in ("lon", "lat"):
        getattr(o, k)[:] = atm[k]
    s.update_atm(atm)
    assert np.array_equal(s.get_cache()["dt"], dt)          # (a re-upload of as many particles keeps cache->dt)
    return o, s


class _Finite:
    """An engine as _compare reads it, with the entries that are not finite in the reference taken out (they are
    compared by class before)."""

    def __init__(self, engine, state, drop):
        self._e, self._s, self._drop = engine, state, drop
        self.ctl, self.cache = engine.ctl, getattr(engine, "cache", None)

    def state(self):
        out = {k: np.array(v) for k, v in self._s.items()}
        for k, m in self._drop.items():
            out[k][m] = 0.0
        return out

    def get_cache(self):
        return self._e.get_cache()


def deviations(g, r, ctl):
    e = {k: cases.rel_err(g[k], r[k]) for k in ("lon", "lat", "p")}
    fin = np.isfinite(r["q"])
    e["q"] = cases.q_rows_err(ctl, np.where(fin, g["q"], 0.0), np.where(fin, r["q"], 0.0))[0] if r["q"].size else 0.0
    return e


def check_module(case, module, o, s, before, tol, tag, states=None):
    """the assertions of the file's head for one module call on both engines (states: their states, if not as stored)"""
    g, r = states or (s.state(), o.state())
    q0 = before["q"].reshape(r["q"].shape)
    changed_r = ~_same(r["p"], before["p"]) | np.any(~_same(r["q"], q0), axis=0) | ~_same(r["lon"], before["lon"]) | ~_same(r["lat"], before["lat"])
    changed_g = ~_same(g["p"], before["p"]) | np.any(~_same(g["q"], q0), axis=0) | ~_same(g["lon"], before["lon"]) | ~_same(g["lat"], before["lat"])
    e = deviations(g, r, o.ctl)
    e.update(acted=int(changed_r.sum()), device_only=int((changed_g & ~changed_r).sum()), oracle_only=int((changed_r & ~changed_g).sum()))
    print("DEPO_EDGE " + json.dumps(dict(tag, case=case["name"], module=module, **e)))
    # untouched by the oracle: the bits the particle came with
    for k in ("p", "lon", "lat"):
        assert np.array_equal(g[k][~changed_r], before[k][~changed_r]), (case["name"], module, k, np.nonzero(changed_g & ~changed_r)[0][:8])
    assert np.array_equal(g["q"][:, ~changed_r], q0[:, ~changed_r], equal_nan=True), (case["name"], module, np.nonzero(changed_g & ~changed_r)[0][:8])
    # acted on by the oracle: acted on by the device
    assert not (changed_r & ~changed_g).any(), (case["name"], module, np.nonzero(changed_r & ~changed_g)[0][:8])
    # the same class where the reference is not finite
    drop = {}
    for k in ("p", "q"):
        bad = ~np.isfinite(r[k])
        assert np.array_equal(np.isnan(g[k]), np.isnan(r[k])), (case["name"], module, k)
        assert np.array_equal(g[k][bad & ~np.isnan(r[k])], r[k][bad & ~np.isnan(r[k])]), (case["name"], module, k)      # +inf / -inf
        drop[k] = bad
    if tol == 0.0:
        for k in KEYS:
            assert np.array_equal(g[k], r[k], equal_nan=True), (case["name"], module, k)
        assert s.get_cache()["rng_ctr"] == o.cache.rng_ctr
    else:
        _compare(_Finite(o, r, drop), _Finite(s, g, drop), tol)
    return g, e


def single_modules(name, tol=TOL, options=None, tag=None):
    """every module of the case from the case's positions on both engines; returns {module: device state}"""
    case = D.all_cases()[name]
    atm = case["atm"]
    out, worst = {}, {}
    for module in case["modules"]:
        o, s = pair(case, options)
        o.module(module)
        s.module(module, case["t"])
        out[module], worst[module] = check_module(case, module, o, s, atm, tol, dict(tag or {}, test="single"))
        s.close()
    return out, worst


@pytest.mark.parametrize("name", NAMES)
def test_single_modules_against_the_oracle(name):
    _default_build_states(name)


@functools.lru_cache(maxsize=None)
def _default_build_states(name):
    return single_modules(name)[0]


SHAPES = {"generic_kernel": dict(generic_kernel=1), "big_grid": dict(big_grid=1)}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("family", FAMILIES)
def test_single_modules_in_other_launch_shapes_have_the_same_bits(family, shape):
    for name in NAMES:
        if name.split("-")[0] != family:
            continue
        base = _default_build_states(name)
        other, _ = single_modules(name, options=SHAPES[shape], tag=dict(shape=shape))
        for module in base:
            for k in KEYS:
                assert np.array_equal(base[module][k], other[module][k], equal_nan=True), (name, module, shape, k)


# ---------------------------------------------------------------------------
# one configuration holding all three modules, through every launch shape of a time step
# ---------------------------------------------------------------------------

RUN_SHAPES = [("default", {}, "steps"), ("generic_kernel", dict(generic_kernel=1), "steps"),
              ("compact_depo_0", dict(compact_depo=0), "steps"), ("compact_depo_1", dict(compact_depo=1), "steps"),
              ("emit_keys_0", dict(emit_keys=0), "steps"), ("emit_keys_1", dict(emit_keys=1), "steps"),
              ("big_grid", dict(big_grid=1), "steps"),
              ("multi_step_on", dict(multi_step=8), "batched"), ("multi_step_off", dict(multi_step=0), "batched")]
RUNS = ("behind_mixing", "fused_tail", "extrap_run-east", "extrap_run-west")


@functools.lru_cache(maxsize=None)
def run_reference(which):
    """(case, oracle behind the third call of the time loop, the step times, launch shapes)"""
    if which.startswith("extrap_run"):
        case = D.extrap_run_case(1 if which.endswith("east") else -1)
        o = B.Oracle(case["ctl"], case["clim"], case["m0"], case["m1"], case["atm"])
        o.timesteps_init()
        times = cases.step_times(o.ctl)[:3]
        for t in times:
            o.run_timestep(t)
        return case, o, times, RUN_SHAPES
    case, o, times, _ = CPU.run_oracle(which == "behind_mixing")
    # SEGMENT particles per workgroup (CPU.test_time_step_case_gives_the_workgroups_the_intended_lists: the lists of the
    # packed-wave launch then have 0, 1, 63, 64, 65 and 257 entries), and once the geometry a run of this size gets by itself
    n = len(case["atm"]["p"])
    blocks = -(-n // D.SEGMENT)
    assert CPU.workgroup_size(n, blocks) == D.SEGMENT
    shapes = [(label, dict(opt, step_blocks=blocks, step_blocks_multi=blocks), mode) for label, opt, mode in RUN_SHAPES]
    return case, o, times, shapes + [("default_geometry", {}, "steps")]


def _by_number(state, case):
    """module_sort permutes the particle arrays (and the device hands them out in that order): back into the case's
    order by the quantity that carries the particle's number"""
    order = np.argsort(state["q"][case["quantities"].index("mloss_decay")].astype(np.int64))
    out = {k: (v[:, order] if k == "q" else v[order]) for k, v in state.items()}
    assert np.array_equal(out["q"][case["quantities"].index("mloss_decay")], np.arange(len(order)))
    return out


def time_steps(which, tol=TOL):
    case, o, times, shapes = run_reference(which)
    atm = case["atm"]
    r = _by_number(o.state(), case)
    runs = {}
    for label, options, mode in shapes:
        s = hip.Simulation(case["ctl"], case["clim"], case["m0"], case["m1"], atm)
        for k, v in options.items():
            s.set_option(k, v)
        s.timesteps_init(atm["time"].min(), atm["time"].max())
        if "bounds" in case:                # the device's bounds are the ones the case placed its particles on
            assert s.shortcuts() == case["bounds"], (s.shortcuts(), case["bounds"])
        if mode == "steps":
            for t in times:
                s.run_timestep(t)
        else:
            s.run_timestep(times[0])
            s.run_timesteps(times[1], len(times) - 1)
        raw = s.state()
        assert np.array_equal(raw["q"][-1], o.state()["q"][-1])             # (the same order on both sides)
        g, e = check_module(case, "time_steps", o, s, atm, tol, dict(test="run", shape=label), (_by_number(raw, case), r))
        runs[label] = g
        s.close()
    first = shapes[0][0]
    for label in runs:
        for k in KEYS:
            assert np.array_equal(runs[label][k], runs[first][k], equal_nan=True), (label, k)
    return r, runs


@pytest.mark.parametrize("which", RUNS)
def test_time_steps_of_all_three_modules_in_every_launch_shape(which):
    """behind_mixing: module_sort and module_mixing in every step, the deposition modules in the packed-wave launch behind
    them (compact_depo, emit_keys); fused_tail: in the tail of the kernel that moves the particles, two steps in one
    launch -- both with particles on the shortcuts' bounds and workgroups that find 0, 1, 63, 64, 65 and 257 particles
    to work on.  extrap_run-*: particles that cross the end of a regional longitude axis within the step."""
    time_steps(which)


def test_which_grids_keep_the_shortcuts():
    """mphip_get_shortcuts on four longitude axes: 0 ... 360 and -180 ... 180 keep the four bounds, an axis that passes for
    periodic but spans a little less than 360 degrees (a float32 axis whose periodic column rounds short) and a regional
    axis have none, the Cartesian twin of the regional axis keeps them."""
    from mptrac_amd.synth import Met
    case = D.all_cases()["skip-min_in_0"]
    m0, m1 = case["m0"], case["m1"]
    want = D.field_bounds(m0, m1, case["ctl"])
    assert all(np.isfinite(v) for v in want.values())
    short = np.linspace(0.0, float(np.float32(359.9)) + float(np.float32(0.1)), 13)
    assert short[-1] - short[0] < 360.0 and abs(short[-1] - short[0] - 360.0) < 0.01
    axes = {"0...360": (m0.lon + 180.0, 0, True), "-180...180": (m0.lon, 0, True), "just short": (short, 0, False),
            "regional": (10.0 + 2.5 * np.arange(13), 0, False), "cartesian": (10.0 + 2.5 * np.arange(13), 1, True),
            "20...380": (m0.lon + 200.0, 0, False)}
    for label, (lon, coord_type, kept) in axes.items():
        mets = [Met(m.time, lon, m.lat, m.p, m.f3, m.f2, coord_type) for m in (m0, m1)]
        s = hip.Simulation(dict(case["ctl"], met_coord_type=coord_type), case["clim"], mets[0], mets[1], case["atm"])
        got = s.shortcuts()
        s.close()
        print("DEPO_EDGE " + json.dumps(dict(test="gate", axis=label, **got)))
        assert got == (want if kept else dict.fromkeys(want, -np.inf)), (label, got)


# ---------------------------------------------------------------------------
# module_radio_depo: depo_pair_factor with sinks that keep the factors
# ---------------------------------------------------------------------------

GROUND = (-180.0, 180.0, 24, -90.0, 90.0, 16)


@pytest.mark.parametrize("case", D.radio_cases(), ids=lambda c: c["name"])
def test_radio_depo_removes_what_the_deposition_modules_remove(case):
    """The planes of the ground inventory show exactly the activity the restatement (tests/refradiodepo.py) removes with
    the oracle's factors: the same particles, the same cells, values within the bar."""
    atm, names = case["atm"], list(case["quantities"])
    n = len(atm["p"])
    # the oracle's factors and whom it acts on, on a mass of one (refradiodepo: inputs of the restatement)
    fac = []
    for module in ("wet_depo", "dry_depo"):
        unit = dict(atm, q=np.array(atm["q"]))
        unit["q"][names.index("m")] = 1.0
        unit["q"][names.index("vmr")] = 1.0
        o, s0 = pair(dict(case, atm=unit))
        s0.close()
        o.module(module)
        aux = o.q[names.index("m")].copy()
        fac += [aux, aux != 1.0]
        dt = o.dt.copy()
    assert max(fac[1].sum(), fac[3].sum()) >= 30, (fac[1].sum(), fac[3].sum())
    idx = [names.index(a) if a in names else -1 for a in RADIO_ACTIVITIES]
    q = np.array(atm["q"])
    ref = RD.Inventory(GROUND).step(case["t"], q, idx, atm["lon"], atm["lat"], dt, *fac)
    options = {}
    if "bounds" in case:                # SEGMENT particles per workgroup: lists of 0, 1, 63, 64, 65 and 257 entries
        blocks = -(-n // D.SEGMENT)
        assert CPU.workgroup_size(n, blocks) == D.SEGMENT
        per_group = CPU.not_skipped(case, atm)[:(n // D.SEGMENT) * D.SEGMENT].reshape(-1, D.SEGMENT).sum(axis=1)
        assert tuple(per_group[-len(D.BUSY_COUNTS):]) == D.BUSY_COUNTS, per_group
        options = dict(step_blocks=blocks)
    o, s = pair(case, options)
    if "bounds" in case:
        got = s.shortcuts()
        assert got["pct"] == case["bounds"]["pct"] and got["ps"] == case["bounds"]["ps"], got
    s.set_radio_decay(names, on=False)
    s.set_radio_depo(GROUND)
    s.module("radio_depo", case["t"])
    g, (t_inv, wet, dry) = s.state(), s.radio_depo()
    s.close()
    assert t_inv == case["t"]
    for k in ("time", "p", "lon", "lat"):
        assert np.array_equal(g[k], atm[k]), k
    worst = 0.0
    for k, name in enumerate(RADIO_ACTIVITIES):
        if name not in names:
            assert not wet[k].any() and not dry[k].any(), name
            continue
        row = names.index(name)
        if name not in RD.DEPOSITING:
            assert np.array_equal(g["q"][row], atm["q"][row]) and not wet[k].any() and not dry[k].any(), name
            continue
        acted = ref.cells >= 0
        assert np.array_equal(g["q"][row][~acted], atm["q"][row][~acted]), name       # untouched: the bits it came with
        assert (g["q"][row] != atm["q"][row])[q[row] != atm["q"][row]].all(), name
        for got, want in ((wet[k], ref.wet[k]), (dry[k], ref.dry[k])):
            assert np.array_equal(got != 0, want != 0), name                          # the same cells
            assert np.array_equal(np.isnan(got), np.isnan(want)), name                # (ps = NaN: a NaN factor on both sides)
            fin = np.isfinite(want)
            if not want[fin].any():
                continue
            top = float(np.max(np.abs(want[fin])))
            worst = max(worst, float(np.max(np.abs(got[fin] - want[fin]))) / top)
        worst = max(worst, cases.rel_err(g["q"][row], q[row]))
    for row, name in enumerate(names):
        if name not in RADIO_ACTIVITIES:
            assert np.array_equal(g["q"][row], atm["q"][row]), name
    print("DEPO_EDGE " + json.dumps(dict(test="radio", case=case["name"], worst=worst)))
    assert worst <= TOL, worst
