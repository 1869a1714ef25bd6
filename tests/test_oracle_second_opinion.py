"""A second opinion on the oracle where no reference-held golden exists (VERDICT r05 "missing" 4): the
modules restated a second time, in numpy, from the text of the reference (tests/refmodules.py, not derived from
oracle/), against the oracle on 1000 particles -- ADVECT 4 with its old-latitude rule (and 2 / 1 through the same
code), both branches of module_diff_turb incl. the displaced latitude of the vertical probes, module_convection,
module_sedi, module_mixing, wet and dry deposition, the boundary-layer closure module_diff_pbl (all three stability
classes), the advection on model levels (zeta / eta: intpol_met_4d_zeta with its level search), module_isosurf, the
region test of module_bound_cond and module_meteo's fields and derived quantities.  Bar: 1e-13 relative (numpy's exp / log / pow are not glibc's)."""
import numpy as np
import pytest

import cases
import refmodules as R
from oracle import binding as B

N = 1000
TOL = 1e-13
DIRECTION = 1       # -1: every case below reversed in time (tests/test_backward_cpu.py runs this file's tests that way)


def _make_case(name, n, seed):
    if DIRECTION == 1:
        return cases.make_case(name, n=n, seed=seed)
    import backward
    ctl, clim, mets, atm = backward.backward_case(name, n, seed=seed)
    return ctl, clim, mets[0], mets[1], atm


def _timesteps(o, t):
    """module_timesteps for the call at time t -- and the inputs of the check that follows: the case runs in this
    file's direction, the particles released before t take a step of that sign, the others none.  Returns who moves."""
    o.module("timesteps", t)
    assert o.ctl.direction == DIRECTION
    released = DIRECTION * (o.time - t) < 0
    assert released.any() and np.all(DIRECTION * o.dt[released] > 0) and np.all(o.dt[~released] == 0)
    return released


def _oracle(name, seed=4711, **over):
    ctl, clim, m0, m1, atm = _make_case(name, N, seed)
    ctl.update(over)
    o = B.Oracle(ctl, clim, m0, m1, atm)
    o.timesteps_init()
    t = cases.step_times(o.ctl)[1]          # (the first call of the time loop has dt = 0)
    assert _timesteps(o, t).all()
    return o, R.Ref(o.ctl, clim, m0, m1), t


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)))


def _qdict(o, names):
    return {k: o.q[getattr(o.ctl, "qnt_" + k)].copy() for k in names if getattr(o.ctl, "qnt_" + k) >= 0}


@pytest.mark.parametrize("advect", [4, 2, 1])
def test_advect_pressure_levels(advect):
    """ADVECT 4 is the headline integrator and appears in no reference test; 2 is pinned by the dd_test golden, so the
    same numpy code agreeing on all three ties the four-stage loop to the pinned one."""
    o, ref, _ = _oracle("advect", advect=advect)
    # a few particles next to the poles and across the date line (DX2DEG's cut-off, FMOD of the longitude)
    o.lat[:4] = (89.9995, -89.9995, 89.99, -89.99)
    o.lon[4:8] = (179.999, -179.999, 359.5, -200.0)
    s0 = (o.time.copy(), o.lon.copy(), o.lat.copy(), o.p.copy())
    o.module("advect")
    time, lon, lat, p = ref.advect(*s0, o.dt.copy())
    assert np.array_equal(time, o.time)
    assert _rel(lon, o.lon) <= TOL and _rel(lat, o.lat) <= TOL and _rel(p, o.p) <= TOL
    assert np.max(np.abs(lon - s0[1])) > 1e-3          # (the particles did move)


def test_old_latitude_rule_is_observable():
    """mptrac.c:3672-3673: only ADVECT 2 converts the final longitude step at the latitude of its last node; the
    restatement with the rule swapped differs from the oracle by far more than the bar -- the check above can see it."""
    o, ref, _ = _oracle("advect", advect=4)
    s0 = (o.time.copy(), o.lon.copy(), o.lat.copy(), o.p.copy())
    o.module("advect")
    orig = R.DX2DEG
    calls = []

    def swapped(dx, lat):
        calls.append(1)
        return orig(dx, lat + 0.01) if len(calls) == 4 else orig(dx, lat)    # the final step at a displaced latitude
    R.DX2DEG = swapped
    try:
        _, lon, _, _ = ref.advect(*s0, o.dt.copy())
    finally:
        R.DX2DEG = orig
    assert _rel(lon, o.lon) > 1e-9


@pytest.mark.parametrize("case,over", [("turb", {}), ("turb", dict(turb_dx_trop=50.0, turb_dx_strat=0.0, turb_dz_strat=0.1)),
                                       ("conv_sedi", {})])
def test_diff_turb_both_branches(case, over):
    o, ref, _ = _oracle(case, **over)
    s0 = (o.time.copy(), o.lon.copy(), o.lat.copy(), o.p.copy())
    o.module("diff_turb")
    rs = o.rs[:3 * N].copy()
    lon, lat, p = ref.diff_turb(*s0, o.dt.copy(), rs)
    assert _rel(lon, o.lon) <= TOL and _rel(lat, o.lat) <= TOL and _rel(p, o.p) <= TOL
    assert np.max(np.abs(p - s0[3])) > 1e-6


def test_vertical_probes_use_the_displaced_latitude():
    """The weights of the two probes of dKz/dz are evaluated after the horizontal part moved the particle
    (mptrac.c:4639-4641 write atm->lat, 4668-4684 read it): with the old latitude the restatement leaves the bar."""
    o, ref, _ = _oracle("turb", turb_dx_trop=5e7, turb_dx_strat=5e7, turb_dz_trop=1.0, turb_dz_strat=0.1)      # (steps of ~100 km)
    s0 = (o.time.copy(), o.lon.copy(), o.lat.copy(), o.p.copy())
    o.module("diff_turb")
    rs = o.rs[:3 * N].copy()
    _, _, p = ref.diff_turb(*s0, o.dt.copy(), rs)
    assert _rel(p, o.p) <= TOL
    tw = ref.tropo_weight
    ref.tropo_weight = lambda t, lat, pp: tw(t, s0[2], pp)       # every weight at the old latitude
    _, _, p_old = ref.diff_turb(*s0, o.dt.copy(), rs)
    assert _rel(p_old, o.p) > 1e-11


@pytest.mark.parametrize("case,over", [("conv_sedi", {}), ("conv_thresh", {}), ("conv_sedi", dict(conv_mix_pbl=0, conv_cape=120.0))])
def test_convection(case, over):
    o, ref, _ = _oracle(case, **over)
    s0 = (o.time.copy(), o.lon.copy(), o.lat.copy(), o.p.copy())
    o.module("convection")
    p = ref.convection(*s0, o.rs[:N].copy())
    assert _rel(p, o.p) <= TOL
    moved = np.count_nonzero(p != s0[3])
    assert 0 < moved < N                       # some particles are mixed, some are not


def test_sedimentation():
    o, ref, _ = _oracle("conv_sedi")
    s0 = (o.time.copy(), o.lon.copy(), o.lat.copy(), o.p.copy())
    rp, rhop = o.q[o.ctl.qnt_rp].copy(), o.q[o.ctl.qnt_rhop].copy()
    o.module("sedi")
    p = ref.sedimentation(*s0, o.dt.copy(), rp, rhop)
    assert _rel(p, o.p) <= TOL and np.max(np.abs(p - s0[3]) / s0[3]) > 1e-9


def test_mixing():
    o, ref, t = _oracle("full", mixing_nx=6, mixing_ny=3, mixing_nz=4)       # (boxes that hold several of the 1000 particles)
    o.time[:] = t                                                            # module_mixing runs behind the movers
    o.time[::50] = 0.0                                                       # ... and leaves out other times
    names = [k for k in ("m", "vmr") if getattr(o.ctl, "qnt_" + k) >= 0]
    o.q[o.ctl.qnt_vmr][:] = np.random.default_rng(5).uniform(1e-10, 3e-9, N)  # (the case starts from a constant ratio)
    rows = [o.q[getattr(o.ctl, "qnt_" + k)].copy() for k in names]
    s0 = (o.time.copy(), o.lon.copy(), o.lat.copy(), o.p.copy())
    o.module("mixing", t)
    new = ref.mixing(t, *s0, rows)
    for k, a, before in zip(names, new, rows):
        got = o.q[getattr(o.ctl, "qnt_" + k)]
        scale = float(np.max(np.abs(got)))
        assert float(np.max(np.abs(a - got))) <= TOL * scale, k
        assert np.count_nonzero(got != before) > N // 2, k


def _scale(o, k, got):
    """a lost mass m (1 - aux) is a small difference of numbers near one: held to the scale of the mass itself"""
    ref_row = o.q[o.ctl.qnt_m] if k.startswith("mloss") else got
    return max(float(np.max(np.abs(ref_row))), 1e-300)


@pytest.mark.parametrize("case", ["full", "wet_henry"])
def test_wet_and_dry_deposition(case):
    o, ref, _ = _oracle(case)
    names = ("m", "vmr", "loss_rate", "mloss_wet", "mloss_dry")
    o.p[::10] = ref.time_2d("ps", o.time, o.lon, o.lat)[::10] - np.linspace(0.0, 40.0, N)[::10]   # some inside the surface layer
    s0 = (o.time.copy(), o.lon.copy(), o.lat.copy(), o.p.copy())
    dt = o.dt.copy()
    q0 = _qdict(o, names)
    o.module("wet_depo")
    act, aux, lam = ref.wet_depo(*s0, dt)
    q1 = ref.apply_loss(q0, act, aux, lam, "mloss_wet")
    assert 0 < np.count_nonzero(act) < N
    for k, v in q1.items():
        got = o.q[getattr(o.ctl, "qnt_" + k)]
        assert float(np.max(np.abs(v - got))) <= TOL * _scale(o, k, got), ("wet", k)
    rp = o.q[o.ctl.qnt_rp].copy() if o.ctl.qnt_rp >= 0 else None
    rhop = o.q[o.ctl.qnt_rhop].copy() if o.ctl.qnt_rhop >= 0 else None
    o.module("dry_depo")
    act, aux, rate = ref.dry_depo(*s0, dt, rp, rhop)
    q2 = ref.apply_loss(q1, act, aux, rate, "mloss_dry")
    assert 0 < np.count_nonzero(act) < N
    for k, v in q2.items():
        got = o.q[getattr(o.ctl, "qnt_" + k)]
        assert float(np.max(np.abs(v - got))) <= TOL * _scale(o, k, got), ("dry", k)


@pytest.mark.parametrize("case,seed", [("pbl", 4711), ("pbl", 99), ("pbl_meso", 7)])
def test_boundary_layer_closure(case, seed):
    """module_diff_pbl (TURB_PBL_SCHEME 1, mptrac.c:4343-4584) appears in no reference test and was "HIP vs oracle only":
    the numpy statement evaluates every particle through all three stability classes and selects as the reference's
    ladder does.  Positions to 1e-13; the single-precision perturbations the module stores must be the oracle's bits."""
    ctl, clim, m0, m1, atm = _make_case(case, 4000, seed)
    o = B.Oracle(ctl, clim, m0, m1, atm)
    o.timesteps_init()
    ts = cases.step_times(o.ctl)
    for t in ts[:3]:                       # a few full steps first: perturbations of every size and sign
        o.run_timestep(t)
    _timesteps(o, ts[3])
    s0 = (o.time.copy(), o.lon.copy(), o.lat.copy(), o.p.copy())
    uv0 = o.uvwp.copy()
    o.module("diff_pbl")
    ref = R.Ref(o.ctl, clim, m0, m1)
    lon, lat, p, uv, act = ref.diff_pbl(*s0, o.dt.copy(), uv0, o.rs[:3 * 4000].copy())
    assert _rel(lon, o.lon) <= TOL and _rel(lat, o.lat) <= TOL and _rel(p, o.p) <= TOL
    assert np.array_equal(uv, o.uvwp)
    assert np.array_equal(act, o.p != s0[3]) or np.count_nonzero(act != (o.p != s0[3])) <= 2      # (a reflected height may land on the old pressure)
    if case == "pbl":
        k = ref.pbl_classes
        assert min(k["neutral"], k["unstable"], k["stable"], k["free_convection_profile"]) > 10, k
    assert 100 < np.count_nonzero(act) < 4000


@pytest.mark.parametrize("case", ["advect_zeta", "advect_zeta_midpoint", "advect_eta"])
def test_advect_model_levels(case):
    """module_advect's zeta / eta branch (mptrac.c:3681-3757) with intpol_met_4d_zeta (2808-2981: the eight column
    searches of locate_vert, the walk to the level pair that brackets the height after the horizontal and time blend, the
    float difference of the two snapshots) -- no reference test runs it, and it was "HIP vs oracle only"."""
    ctl, clim, m0, m1, atm = _make_case(case, 3000, 4711)
    o = B.Oracle(ctl, clim, m0, m1, atm)
    o.timesteps_init()
    ts = cases.step_times(o.ctl)
    for t in ts[:2]:
        o.run_timestep(t)
    _timesteps(o, ts[2])
    s0 = (o.time.copy(), o.lon.copy(), o.lat.copy(), o.p.copy())
    o.module("advect")
    ref = R.Ref(o.ctl, clim, m0, m1)
    time, lon, lat, p, zeta = ref.advect_ml(*s0, o.dt.copy())
    row = o.ctl.qnt_zeta if o.ctl.advect_vert_coord == 1 else o.ctl.qnt_eta
    assert np.array_equal(time, o.time)
    assert _rel(lon, o.lon) <= TOL and _rel(lat, o.lat) <= TOL and _rel(p, o.p) <= TOL and _rel(zeta, o.q[row]) <= TOL
    assert np.max(np.abs(lon - s0[1])) > 1e-3 and np.max(np.abs(p - s0[3])) > 1e-3
    assert ref.ml_walked > 0          # some stencils needed the walk beyond the lowest of the eight column indices


@pytest.mark.parametrize("case", ["isosurf_p", "isosurf_rho", "isosurf_theta", "isosurf_balloon"])
def test_isosurface_modes(case):
    """module_isosurf_init stores pressure / density / potential temperature, module_isosurf puts the particle back on
    that surface after the movers (mptrac.c:4886-5005); mode 4 follows a balloon's pressure record."""
    ctl, clim, m0, m1, atm = _make_case(case, N, 11)
    o = B.Oracle(ctl, clim, m0, m1, atm)
    cases.prepare(o)
    o.timesteps_init()
    ts = cases.step_times(o.ctl)
    released = _timesteps(o, ts[1])
    assert not released[::7].any() and np.all(o.dt[::7] == 0) and released.sum() == N - len(o.dt[::7])   # the late release
    ref = R.Ref(o.ctl, clim, m0, m1)
    s0 = (o.time.copy(), o.lon.copy(), o.lat.copy(), o.p.copy())
    if o.ctl.isosurf != 4:
        o.module("isosurf_init")
        iso = ref.isosurf_init(*s0)
        assert _rel(iso, o.iso_var) <= TOL
    else:
        iso = None
    o.module("advect")
    s1 = (o.time.copy(), o.lon.copy(), o.lat.copy(), o.p.copy())
    o.module("isosurf")
    p = ref.isosurf(*s1, iso, balloon=cases.BALLOON)
    assert _rel(p, o.p) <= TOL
    if o.ctl.isosurf != 1:
        assert np.max(np.abs(o.p - s0[3])) > 1e-6


@pytest.mark.parametrize("case", ["bound", "bound_pbl_zeta"])
def test_boundary_condition_region_and_values(case):
    """module_bound_cond (mptrac.c:3789-3881): latitude / pressure box, surface layer by pressure depth, height, zeta and
    boundary-layer top; mass and volume mixing ratio with their trends, age of air."""
    ctl, clim, m0, m1, atm = _make_case(case, N, 5)
    o = B.Oracle(ctl, clim, m0, m1, atm)
    o.timesteps_init()
    ts = cases.step_times(o.ctl)
    _timesteps(o, ts[1])
    ref = R.Ref(o.ctl, clim, m0, m1)
    o.p[::7] = ref.time_2d("ps", o.time, o.lon, o.lat)[::7] - np.linspace(0.0, 60.0, N)[::7]      # some next to the ground
    s0 = (o.time.copy(), o.lon.copy(), o.lat.copy(), o.p.copy())
    before = o.q.copy()
    o.module("bound_cond")
    inside, mass, vmr, age = ref.bound_cond(*s0)
    assert 0 < np.count_nonzero(inside) < N
    for row, new in ((o.ctl.qnt_m, mass), (o.ctl.qnt_vmr, vmr), (o.ctl.qnt_aoa, age)):
        if row >= 0 and new is not None:
            want = np.where(inside, new, before[row])
            assert np.allclose(o.q[row], want, rtol=1e-15, atol=0.0), row
            assert np.array_equal(o.q[row] != before[row], inside & (want != before[row]))


@pytest.mark.parametrize("case", ["advect_mlp", "advect_mlp_midpoint"])
def test_advect_pressure_with_model_level_winds(case):
    """ADVECT_VERT_COORD 2 (mptrac.c:3647-3657): the pressure-level integrator with u, v, omega from the model levels,
    located by the level pressures through intpol_met_4d_zeta."""
    o, ref, _ = _oracle(case)
    s0 = (o.time.copy(), o.lon.copy(), o.lat.copy(), o.p.copy())
    o.module("advect")
    time, lon, lat, p = ref.advect(*s0, o.dt.copy())
    assert np.array_equal(time, o.time)
    assert _rel(lon, o.lon) <= TOL and _rel(lat, o.lat) <= TOL and _rel(p, o.p) <= TOL
    assert np.max(np.abs(lon - s0[1])) > 1e-3


@pytest.mark.parametrize("case", ["meteo", "meteo_gated"])
def test_meteo_fields_and_derived_quantities(case):
    """module_meteo (mptrac.c:5062-5165): every interpolated field and every derived quantity the two cases carry -- the
    humidity macros, potential temperature, the diagnosed zeta, virtual temperature, the moist lapse rate (RA SQR(t):
    the square first), dew and frost point."""
    o, ref, _ = _oracle(case)
    names = cases.CASE_QUANTITIES[case]
    o.module("meteo")
    want = ref.meteo(o.time.copy(), o.lon.copy(), o.lat.copy(), o.p.copy())
    checked = 0
    for row, name in enumerate(names):
        if name in ("m", "rp", "rhop"):
            continue
        assert name in want, name
        got = o.q[row]
        fin = np.isfinite(got)                      # (sst is NaN over land: the nearest-corner rule on both sides)
        assert np.array_equal(fin, np.isfinite(want[name])), name
        scale = max(float(np.max(np.abs(got[fin]))), 1e-300)
        assert float(np.max(np.abs(want[name][fin] - got[fin]))) <= TOL * scale, name
        assert np.ptp(got[fin]) > 0, name
        checked += 1
    assert checked == len(names) - sum(n in ("m", "rp", "rhop") for n in names)


def test_sort_keys_and_a_stable_order():
    """module_sort's box index (mptrac.c:5913-5919: locate_reg on the longitude as it is, not wrapped) and the order it
    induces; ties keep their index order here (GSL's gsl_sort_index leaves them unspecified)."""
    o, ref, _ = _oracle("full")
    o.lon[:6] = (-190.0, 185.0, 359.9, -180.0, 179.99999, 540.0)          # outside the axis: the end cells
    for k in (400, 20, 777):                                              # ... and three particles in the box of a fourth: ties
        o.lon[k], o.lat[k], o.p[k] = o.lon[50] + 1e-3, o.lat[50] - 1e-3, o.p[50] * (1.0 + 1e-5)
    lon, lat, p, q0 = o.lon.copy(), o.lat.copy(), o.p.copy(), o.q.copy()
    keys, perm = o.sort()
    want = ref.sort_keys(lon, lat, p)
    assert np.array_equal(keys, want)
    order = np.argsort(want, kind="stable")
    assert np.array_equal(perm, order)
    assert np.array_equal(o.lon, lon[order]) and np.array_equal(o.p, p[order]) and np.array_equal(o.q, q0[:, order])
    assert len(np.unique(want)) <= len(want) - 3                          # (the ties are there)
