"""The stable radix sort (sort_hist_kernel, sort_scan_local_kernel, sort_scan_chunks_kernel, sort_scatter_kernel) and the
order repair (repair_count_kernel, repair_scan_kernel, repair_split_kernel, the radix sort of the movers whose count lives
on the device, repair_merge_kernel) on inputs placed by key (tests/sort_cases.py): every pass plan and digit width, digit
runs that coincide with and straddle a round, a wave's share and a tile, valid keys in the digit of the padding lanes,
counters on both sides of the scan's chunk border, and mover patterns on the borders of the repair's tiles.

Reference: numpy's stable argsort of the placed keys (ties by index), and the CPU oracle, which
tests/test_sort_edges_cpu.py holds against it on the same inputs.  Keys, permutations, masses and the counter of the random
numbers are compared with array_equal; positions against the oracle within the project's 1e-10
(tests/test_gpu_parity.py:_compare), between the runs with and without the repair with array_equal.  Every repair test
asserts how many module_sort calls the repair answered (Simulation.sort_counts).

Every comparison prints one "SORT_EDGE {json}" line before it asserts.  tests/test_gpu_sort_edges_exact.py repeats a
part in the reference-rounding build with tolerance 0, through the functions of this file."""
import json
import time

import numpy as np
import pytest

import cases
import sort_cases as S
from mptrac_amd import hip
from oracle import binding as B

pytestmark = pytest.mark.gpu

TOL = 1e-10          # north_star tolerance for positions
ARRAYS = ("time", "lon", "lat", "p", "q")


def _gathered(atm, perm):
    return {k: np.asarray(atm[k])[..., perm] for k in ARRAYS}


def _equal(a, b, keys=ARRAYS):
    return {k: bool(np.array_equal(a[k], b[k])) for k in keys}


# ---------------------------------------------------------------------------
# from scratch
# ---------------------------------------------------------------------------

def scratch(case):
    """Simulation.sort() of one placed case: sorted keys, permutation and every array against the stable argsort and the
    oracle; a second sort returns the same keys and the identity."""
    grid, pattern, n, bits = case
    keys = S.pattern_keys(grid, pattern, n, bits)
    ctl, clim, m0, m1, atm = S.scratch_inputs(grid, keys)
    ref = np.argsort(keys, kind="stable")
    o = B.Oracle(ctl, clim, m0, m1, atm)
    keys_o, perm_o = o.sort()
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    if bits:
        s.set_option("sort_bits", bits)
    t0 = time.perf_counter()
    keys_s, perm_s = s.sort()
    g = s.state()
    keys_2, perm_2 = s.sort()
    g2 = s.state()
    seconds = time.perf_counter() - t0
    counts = s.sort_counts()
    s.close()
    P = S.plan(grid, n, bits)
    row = dict(test="scratch", case=S.case_id(case), passes=P["passes"], bits=P["bits"], pair=P["pair"], tiles=P["ntiles"],
               chunks=P["nchunks"], keys=bool(np.array_equal(keys_s, keys[ref])), perm=bool(np.array_equal(perm_s, ref)),
               oracle=bool(np.array_equal(keys_o, keys) and np.array_equal(perm_o, perm_s)),
               state=_equal(g, _gathered(atm, ref)), again=bool(np.array_equal(keys_2, keys_s)
                                                                 and np.array_equal(perm_2, np.arange(n))),
               state_again=_equal(g2, g), counts=counts, seconds=round(seconds, 4))
    print("SORT_EDGE " + json.dumps(row))
    assert row["keys"] and row["perm"] and row["oracle"] and row["again"], row
    assert all(row["state"].values()) and all(row["state_again"].values()), row
    assert np.array_equal(g["q"][0], ref + 1.0)              # the mass is the original index + 1
    assert counts == (0, 2)                                  # module_sort on its own never repairs
    return row


@pytest.mark.parametrize("case", [c + (0,) for c in S.SCRATCH], ids=S.case_id)
def test_placed_keys_with_the_automatic_digit_width(case):
    scratch(case)


@pytest.mark.parametrize("case", S.FORCED, ids=S.case_id)
def test_placed_keys_with_a_forced_digit_width(case):
    scratch(case)


def test_sort_from_an_internal_order():
    """locality_sort_interval 1: after two time steps (the second one moves every particle) the particles are stored in
    the internal locality order, which module_sort undoes first (restore_external_order).  Keys and permutation of the
    oracle's module_sort on the device's state, which is numpy's stable argsort of those keys.  The positions in front of
    the sort are read with get_atm, which leaves the stored order alone (get_cache with arrays would restore the
    caller's order itself); Simulation.sorts_undone counts the module_sort calls that met the internal order, and the
    second sort() of the test, which starts from the sorted caller's order, is the one that does not."""
    grid, n = "p2b8", 8193
    ctl, clim, m0, m1, atm = S.scratch_inputs(grid, S.pattern_keys(grid, "tied", n))
    s = hip.Simulation(ctl, clim, m0, m1, atm)
    s.set_option("locality_sort_interval", 1)
    s.timesteps_init(0.0, 0.0)
    for t in cases.step_times(s.ctl)[:2]:
        s.run_timestep(t)
    g = s.get_atm()
    assert np.count_nonzero(g["lon"] != atm["lon"]) > n // 2 and np.array_equal(g["q"], atm["q"])
    o = B.Oracle(ctl, clim, m0, m1, {k: g[k] for k in ARRAYS})
    keys_o, perm_o = o.sort()
    undone = [s.sorts_undone()]
    keys_s, perm_s = s.sort()
    undone.append(s.sorts_undone())
    sorted_state = s.state()
    keys_2, perm_2 = s.sort()
    undone.append(s.sorts_undone())
    counts = s.sort_counts()
    s.close()
    ref = np.argsort(keys_o, kind="stable")
    row = dict(test="internal_order", keys=bool(np.array_equal(keys_s, keys_o[ref])), perm=bool(np.array_equal(perm_s, ref)),
               oracle=bool(np.array_equal(perm_o, ref)), state=_equal(sorted_state, _gathered(g, ref)),
               again=bool(np.array_equal(keys_2, keys_s) and np.array_equal(perm_2, np.arange(n))),
               distinct=int(len(np.unique(keys_o))), undone=undone, counts=counts)
    print("SORT_EDGE " + json.dumps(row))
    assert row["keys"] and row["perm"] and row["oracle"] and row["again"] and all(row["state"].values()), row
    assert np.any(np.diff(keys_o) < 0) and row["distinct"] < n          # (unsorted, with ties)
    assert undone == [0, 1, 1] and counts == (0, 2), row              # the first sort() met the internal order


# ---------------------------------------------------------------------------
# the repair
# ---------------------------------------------------------------------------

def _device_runs(case, inputs, keep_before=False):
    """the case with sort_repair 1 and 0: per step keys and permutation of module_sort, state, counter, sort counts"""
    runs = {}
    for repair in (1, 0):
        s = hip.Simulation(*inputs)
        s.set_option("sort_repair", repair)
        s.timesteps_init(inputs[4]["time"].min(), inputs[4]["time"].max())
        rows = []
        for t in S.step_times(case):
            before = s.get_atm() if keep_before else None
            t0 = time.perf_counter()
            s.run_timestep(t)
            keys, perm = s.get_sort()
            seconds = time.perf_counter() - t0
            state = s.state()
            rows.append(dict(keys=keys.astype(np.int64), perm=perm, state=state, ctr=s.get_cache()["rng_ctr"],
                             counts=s.sort_counts(), before=before, seconds=seconds))
        s.close()
        runs[repair] = rows
    return runs


def _check_steps(name, runs, refs, tol, oracle):
    """refs: per step dict(keys by slot before the sort, perm, movers[, state, ctr])"""
    for k, ref in enumerate(refs):
        a, b = runs[1][k], runs[0][k]
        stable = np.argsort(ref["keys"], kind="stable")
        row = dict(test="repair", case=name, step=k, movers=int(ref["movers"].sum()), counts=a["counts"], counts_off=b["counts"],
                   stable=bool(np.array_equal(ref["perm"], stable)))
        for tag, run in (("on", a), ("off", b)):
            row["keys_" + tag] = bool(np.array_equal(run["keys"], ref["keys"][stable]))
            row["perm_" + tag] = bool(np.array_equal(run["perm"], stable))
        row["runs"] = _equal(a["state"], b["state"], ARRAYS + ("uvwp",))
        row["ctr"] = bool(a["ctr"] == b["ctr"])
        if oracle:
            r = ref["state"]
            row["oracle"] = {c: cases.rel_err(a["state"][c], r[c]) for c in ("lon", "lat", "p")}
            row["oracle_exact"] = _equal(a["state"], r, ("time", "q", "uvwp"))
            row["oracle_ctr"] = bool(a["ctr"] == ref["ctr"])
        row["seconds"] = round(a["seconds"], 4)
        print("SORT_EDGE " + json.dumps(row))
        assert row["stable"] and row["keys_on"] and row["perm_on"] and row["keys_off"] and row["perm_off"], row
        assert all(row["runs"].values()) and row["ctr"], row
        if oracle:
            assert all(row["oracle_exact"].values()) and row["oracle_ctr"], row
            assert all(e <= tol for e in row["oracle"].values()), row
        # the first module_sort sorts from scratch, every later one repairs -- or none does
        assert a["counts"] == (k, 1) and b["counts"] == (0, k + 1), row


def repair(name, tol=TOL):
    case = S.repair_case(name)
    refs = S.oracle_run(name)
    runs = _device_runs(case, S.repair_inputs(case))
    _check_steps(name, runs, refs, tol, oracle=True)
    assert sum(int(r["movers"].sum()) for r in refs) > 0 or name == "none"
    assert np.array_equal(np.sort(runs[1][-1]["state"]["q"][0]), np.arange(1.0, case["n"] + 1.0))      # nobody lost or doubled


@pytest.mark.parametrize("name", S.REPAIR)
def test_repair_equals_the_stable_sort_at_every_step(name):
    repair(name)


def test_repair_with_two_tiles_per_thread_of_its_scan():
    """n = 1 049 601 (1026 tiles, repair_scan_kernel with per = 2), three steps, about 15 % movers in the last sort:
    against numpy's stable argsort of the keys of the positions in front of every step and the run without the repair.
    The keys are those of sort_cases.model_run, which tests/test_sort_edges_cpu.py holds against the oracle at the
    smaller sizes."""
    case = S.repair_case(S.BIG)
    t0 = time.perf_counter()
    runs = _device_runs(case, S.repair_inputs(case), keep_before=True)
    device_seconds = time.perf_counter() - t0
    model = S.model_run(case)
    refs = []
    for k, m in enumerate(model):
        before = runs[0][k]["before"]
        keys = S.keys_of(case["grid"], before["lon"], before["lat"], before["p"])
        assert np.array_equal(keys, m["keys"]), k
        for r in (0, 1):
            assert all(np.array_equal(runs[r][k]["before"][c], before[c]) for c in ARRAYS), (k, r)
        refs.append(dict(keys=keys, perm=m["perm"], movers=m["movers"]))
    print("SORT_EDGE " + json.dumps(dict(test="repair_big", n=case["n"], device_seconds=round(device_seconds, 3),
                                         sort_steps=[round(r["seconds"], 4) for r in runs[1]])))
    _check_steps(S.BIG, runs, refs, TOL, oracle=False)
    assert 0.14 * case["n"] < refs[2]["movers"].sum() < 0.16 * case["n"]


def test_a_new_particle_set_is_sorted_from_scratch():
    """The repair needs the particles stored in the order of the last module_sort: after mphip_update_atm with the same
    number of particles and after a particle set of another size the next module_sort sorts from scratch, the one behind
    it repairs again.  Same bits as the run without the repair throughout."""
    case, other = S.repair_case("n2049"), S.repair_case("n1025")
    inputs, atm_other = S.repair_inputs(case), S.repair_inputs(other)[4]
    times = [k * S.CTL["dt_mod"] for k in range(6)]
    expect = [(0, 1), (1, 1), (1, 2), (2, 2), (2, 3), (3, 3)]
    runs = {}
    for rep in (1, 0):
        s = hip.Simulation(*inputs)
        s.set_option("sort_repair", rep)
        s.timesteps_init(0.0, S.NEVER)
        rows = []
        for k, t in enumerate(times):
            if k == 2:
                s.update_atm(inputs[4])
            if k == 4:
                s.replace_particles(atm_other)
            s.run_timestep(t)
            keys, perm = s.get_sort()
            rows.append(dict(keys=keys, perm=perm, state=s.state(), ctr=s.get_cache()["rng_ctr"], counts=s.sort_counts()))
        s.close()
        runs[rep] = rows
    for k in range(len(times)):
        a, b = runs[1][k], runs[0][k]
        row = dict(test="new_particles", step=k, counts=a["counts"], counts_off=b["counts"],
                   sort=bool(np.array_equal(a["keys"], b["keys"]) and np.array_equal(a["perm"], b["perm"])),
                   runs=_equal(a["state"], b["state"], ARRAYS + ("uvwp",)), ctr=bool(a["ctr"] == b["ctr"]))
        print("SORT_EDGE " + json.dumps(row))
        assert row["sort"] and all(row["runs"].values()) and row["ctr"], row
        assert a["counts"] == expect[k] and b["counts"] == (0, k + 1), row
        assert np.all(np.diff(a["keys"]) >= 0)
    assert np.any(runs[1][3]["perm"] != np.arange(case["n"])) and np.any(runs[1][5]["perm"] != np.arange(other["n"]))
