"""The internal locality re-sort folded into the multi-step launch that follows it (mphip_run_timesteps, option
fold_resort, DevAtm::perm_all): the launch reads its per-launch loads -- time, position, the mesoscale perturbations,
dt, the external index and every quantity row -- through the sort's permutation instead of a gather pass of its own in
front of a single-step launch.  Nothing observable may change: every case runs with the fold, without it
(fold_resort 0: the stand-alone gather) and as single mphip_run_timestep calls, and compares the bits of time, lon,
lat, p, uvwp, EVERY quantity row, cache->dt and the random-number counter, downloaded in the caller's order.

locality_sort_interval is 3, so that re-sorts fall inside short calls.  With the particles in the caller's order at
the start, a call of mphip_run_timesteps(DT, K) then runs (S = a single-step launch behind a stand-alone sort, [..] =
one multi-step launch, f = with the folded re-sort):

    fold_resort 0:  S1 [2 3] S4 [5 6] S7 [8 9] S10 ...      the re-sort's step always alone
    fold_resort 1:  S1 [2 3] f[4 5 6] f[7 8 9] S10 ...      S1: the first sort out of the caller's order is a random
                                                             permutation (records), never folded; S10 of a 10-step call:
                                                             one step left, the fallback

Every particle has its own rp, rhop and m: a value that arrives in another particle's slot moves p or shows in m.

Break checks, each tried once on a scratch copy of the kernel (profiles/r07_fold_resort_ab.txt lists the failing tests):
the external index not composed with the one in place, cache->dt not moved, uvwp gathered from slot i.
"""
import numpy as np
import pytest

import cases
from mptrac_amd import hip

pytestmark = pytest.mark.gpu

DT = cases.BASE["dt_mod"]
STATE = ("time", "lon", "lat", "p", "uvwp", "q", "dt")
GRID = dict(grid_nx=36, grid_ny=18, grid_nz=2, grid_z0=0.0, grid_z1=30.0)


def _inputs(n, release=None, decay=False, case="conv_sedi"):
    ctl, clim, m0, m1, atm = cases.make_case(case, n=n)
    ctl = dict(ctl, **GRID)
    if decay:       # module_decay in the launch's tail: writes m, loss_rate, mloss_decay at slot i behind the gather
        ctl = dict(ctl, tdec_trop=259200.0, tdec_strat=259200.0)
    rng = np.random.default_rng(20240919)
    q = list(cases.QUANTITIES)
    atm["q"][q.index("rp")] = rng.uniform(1.0, 20.0, n)
    atm["q"][q.index("rhop")] = rng.uniform(500.0, 2000.0, n)
    atm["q"][q.index("m")] = rng.permutation(n) + 1.0
    if release is not None:     # every seventh particle is released later: dt = 0 for it in the steps before
        atm["time"][::7] = release * DT
    return ctl, clim, m0, m1, atm


def _run(inputs, calls, mode, interval=3, blocks=None, grid_t=None, store_dt=None):
    """mode: "fold", "nofold" (mphip_run_timesteps with fold_resort 1 / 0) or "single" (mphip_run_timestep calls).
    calls: (first step number, steps) of each mphip_run_timesteps call; store_dt: module_timesteps alone at that step
    number first.  Returns the state, the step-kernel launches
    of every call and (grid_t given) the gridded sums."""
    ctl, clim, m0, m1, atm = inputs
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    try:
        s.set_option("locality_sort_interval", interval)
        s.set_option("fold_resort", 1 if mode == "fold" else 0)
        if blocks:
            s.set_option("step_blocks_multi", blocks)
        s.timesteps_init(float(atm["time"].min()), float(atm["time"].max()))
        if store_dt is not None:      # module_timesteps alone stores cache->dt (no launch of the calls below does)
            s.module("timesteps", store_dt * DT)
        launches = []
        for first, nsteps in calls:
            s.profile_begin()
            if mode == "single":
                for k in range(nsteps):
                    s.run_timestep((first + k) * DT)
            else:
                s.run_timesteps(first * DT, nsteps)
            launches.append(s.profile_end()[0])
        g = s.state()
        cache = s.get_cache()
        g["dt"] = cache["dt"]
        g["rng_ctr"] = cache["rng_ctr"]
        g["launches"] = launches
        if grid_t is not None:
            g["grid"] = s.grid_sums(grid_t * DT)
    finally:
        s.close()
    return g


def _same(a, b, what):
    assert a["rng_ctr"] == b["rng_ctr"], what
    for k in STATE:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _three_ways(inputs, calls, **kw):
    fold = _run(inputs, calls, "fold", **kw)
    nofold = _run(inputs, calls, "nofold", **kw)
    single = _run(inputs, calls, "single", **kw)
    _same(fold, nofold, "fold / stand-alone gather")
    _same(fold, single, "fold / single steps")
    return fold, nofold, single


_CASE1 = {}


def _case1():
    """n = 1000 (the last workgroup is partial), ten steps in one call; computed once."""
    if not _CASE1:
        inputs = _inputs(1000)
        _CASE1["inputs"] = inputs
        for mode in ("fold", "nofold", "single"):
            _CASE1[mode] = _run(inputs, [(1, 10)], mode, grid_t=10)
    return _CASE1


def test_ten_steps_three_ways():
    c = _case1()
    _same(c["fold"], c["nofold"], "fold / stand-alone gather")
    _same(c["fold"], c["single"], "fold / single steps")
    assert np.all(c["fold"]["time"] == 10 * DT)
    q = list(cases.QUANTITIES)      # (what no module writes comes back as it went in, in the caller's slots)
    for name in ("m", "rp", "rhop"):
        assert np.array_equal(c["fold"]["q"][q.index(name)], c["inputs"][4]["q"][q.index(name)]), name


def test_launch_counts_show_the_fold():
    # the schedule of the module's docstring: 1 + 3 x (1 + 1) = 7 launches without the fold (S1 [2 3] S4 [5 6] S7 [8 9]
    # S10), 5 with it (S1 [2 3] f[4 5 6] f[7 8 9] S10), 10 step by step
    c = _case1()
    assert c["nofold"]["launches"] == [7]
    assert c["fold"]["launches"] == [5]
    assert c["single"]["launches"] == [10]


def test_gridded_output_does_not_see_the_fold():
    c = _case1()
    for a, b in zip(c["fold"]["grid"], c["nofold"]["grid"]):
        assert np.array_equal(a, b, equal_nan=True)
    assert c["fold"]["grid"][0].sum() > 0


def test_no_resort_at_all_gives_the_same_bits():
    # locality_sort_interval 0: the particles stay in the caller's order -- the order is not observable
    c = _case1()
    fold, nofold, single = _three_ways(c["inputs"], [(1, 10)], interval=0)
    _same(fold, c["fold"], "no re-sort / re-sort every 3 steps")
    assert fold["launches"] == [1]      # [1 ... 10]: without a sort in front of it the first step shares the launch


def test_a_thread_that_walks_two_particles():
    # eight logical blocks of 512 particles (the last ones short or empty): a thread gathers a second particle and
    # reuses its parking slot
    fold, nofold, single = _three_ways(_inputs(3000), [(1, 10)], blocks=8)
    assert fold["launches"] == [5] and nofold["launches"] == [7]


@pytest.mark.parametrize("release", [2.5, 4.5])
def test_particles_released_later(release):
    # 2.5 DT: dt = 0 in the steps in front of the first fold; 4.5 DT: they start inside the folded launch [4 5 6]
    fold, nofold, single = _three_ways(_inputs(1000, release=release), [(1, 10)])
    assert np.all(fold["time"][::7] == 10 * DT)      # (they did start)
    assert fold["launches"] == [5]


def test_particles_that_never_start():
    # released behind the last step: dt = 0 in every step of both folded launches -- they come back with what they were
    # loaded with, through two permutations, in their external slots
    inputs = _inputs(1000, release=12.5)
    fold, nofold, single = _three_ways(inputs, [(1, 10)])
    assert fold["launches"] == [5]
    late = np.zeros(1000, dtype=bool)
    late[::7] = True
    assert np.all(fold["time"][late] == 12.5 * DT)
    assert np.all(fold["dt"][late] == 0)
    for k in ("lon", "lat", "p"):
        assert np.array_equal(fold[k][late], inputs[4][k][late]), k
    assert np.array_equal(fold["q"][:, late], inputs[4]["q"][:, late])
    assert np.all(fold["time"][~late] == 10 * DT)


def test_stored_dt_moves_with_the_particles():
    # cache->dt as module_timesteps at 3 DT left it (t - time: 0.5 DT for every seventh particle, released at 2.5 DT,
    # 3 DT for the others) is written by no launch of the call (none carries a store of dt): it comes back where it was
    inputs = _inputs(1000, release=2.5)
    fold, nofold, single = _three_ways(inputs, [(1, 10)], store_dt=3)
    assert fold["launches"] == [5]
    want = np.full(1000, 3 * DT)
    want[::7] = 0.5 * DT
    assert np.array_equal(fold["dt"], want)


@pytest.mark.parametrize("case", ["pbl_meso", "advect", "advect_midpoint"])
def test_the_other_lean_instantiations(case):
    # conv_sedi runs the instantiation that parks the external index; these do not park.  pbl_meso: the boundary-layer
    # closure's instantiation, which moves uvwp, dt and the external index in a call and reads slot i back (and draws its
    # random numbers by the index it reads back in every step); advect, advect_midpoint: four and two stages without
    # module_diff_meso -- uvwp is stored by the move itself, not behind the last step
    fold, nofold, single = _three_ways(_inputs(1000, case=case), [(1, 10)], store_dt=3)
    assert fold["launches"] == [5] and nofold["launches"] == [7]
    assert np.all(fold["time"] == 10 * DT)
    assert np.all(fold["dt"] == 3 * DT)


def test_one_step_left_takes_the_fallback():
    # S1 [2 3] S4: the re-sort falls due with one step left -- a stand-alone gather and a single-step launch either way
    fold, nofold, single = _three_ways(_inputs(1000), [(1, 4)])
    assert fold["launches"] == [3] and nofold["launches"] == [3]


def test_two_steps_the_smallest_fold():
    # S1 [2 3] | f[4 5]  against  S1 [2 3] | S4 [5]
    fold, nofold, single = _three_ways(_inputs(1000), [(1, 3), (4, 2)])
    assert fold["launches"] == [2, 1]
    assert nofold["launches"] == [2, 2]


def test_two_resorts_in_one_call_compose_the_external_index():
    # S1 [2 3] f[4 5 6] f[7 8]: the external index goes through the first sort's and both folds' permutations
    fold, nofold, single = _three_ways(_inputs(1000), [(1, 8)])
    assert fold["launches"] == [4]       # S1 [2 3] f[4 5 6] f[7 8]
    assert nofold["launches"] == [6]     # S1 [2 3] S4 [5 6] S7 [8]


def test_tail_module_behind_the_gather():
    # module_decay runs in the launch's tail, on m / loss_rate / mloss_decay at slot i, which the gather wrote
    inputs = _inputs(1000, decay=True)
    fold, nofold, single = _three_ways(inputs, [(1, 10)])
    assert fold["launches"] == [5]
    q = list(cases.QUANTITIES)
    m0 = inputs[4]["q"][q.index("m")]
    m = fold["q"][q.index("m")]
    assert np.all(m < m0) and np.all(m > 0.99 * m0)      # 1800 s of a three-day e-folding time, every particle its own m
    assert np.array_equal(np.argsort(m), np.argsort(m0))
