"""The box-edge inputs (tests/box_cases.py) on the reference alone: they reach what they are meant to reach -- faces
whose own coordinate falls into the cell below, the guard `ix >= nx` deciding below an upper bound, particles on either
side of every bound and of both ends of the time window, occupied cells either side of every placed face, pressures
whose height is a face's to the bit -- and the references the device tests use agree with each other on them: the
oracle's module_mixing with its numpy restatement, Oracle.grid_sums with refanalysis.box_sums.  No GPU."""
import json
import math

import numpy as np
import pytest

import box_cases as BC
import refanalysis as RA
import refmodules as RM
from oracle import binding as B

T, DT = BC.T, BC.DT_MOD


@pytest.fixture(scope="module", params=list(BC.GRIDS))
def case(request):
    name = request.param
    atm, npl, tags = BC.particles(name, T, DT)
    facts, cell = BC.facts(name, atm, tags, T, DT)
    print("BOX_CASE " + json.dumps(facts))
    return name, atm, npl, tags, facts, cell


def test_faces_in_the_lower_cell_and_the_guard(case):
    name, atm, npl, tags, facts, cell = case
    # Where the arithmetic draws a cell's border is not where lo + k d lies: an interior face's own point in cell k - 1
    # (grid A: on every axis), or the double below a face already in cell k (grid B; measured there: no face of its three
    # axes (0, 360, 49), (-43, 127, 17), (0, 24, 7) falls into the lower cell, 3 and 12 doubles below a face lie in the
    # upper one).  box_cases.threshold places the two doubles either side of the border itself for every face.
    if name == "B":
        assert sum(n for n, _ in facts["face_in_lower_cell"].values()) == 0, facts
        assert facts["below_in_upper_cell"]["lon"][0] >= 1 and facts["below_in_upper_cell"]["lat"][0] >= 1, facts
    if name == "A":
        assert facts["face_in_lower_cell"] == {"lon": (2, 7), "lat": (1, 11), "z": (1, 9)}, facts
        assert all(v >= 1 for v in facts["guard_decides"].values()), facts
    if name == "C":
        # x < hi with a quotient == n exists one double below 180 and below 90.  On the z axis (-5, 85, 90) the width is 1
        # and Z + 5 is exact below 85 (85 and 90 share a binade), so no height below 85 has the quotient 90: the guard
        # cannot decide there, whatever the input
        assert facts["guard_decides"]["lon"] >= 1 and facts["guard_decides"]["lat"] >= 1, facts
        assert facts["guard_decides"]["z"] == 0 and (math.nextafter(85.0, 0.0) + 5.0) / 1.0 < 90.0
    # a face that falls into the lower cell is placed, and the reference puts it there
    for i, tg in enumerate(tags):
        if tg[0] == "face" and tg[3] == 0 and tg[1] < 2 and 0 < tg[2] < BC.axis(BC.GRIDS[name], tg[1])[2]:
            k = BC.decompose(BC.GRIDS[name], int(cell[i]))[tg[1]]
            assert k == BC.index(BC.GRIDS[name], tg[1], BC.face(BC.GRIDS[name], tg[1], tg[2])) and k in (tg[2] - 1, tg[2])


def test_bounds_and_window_ends(case):
    name, atm, npl, tags, facts, cell = case
    grid = BC.GRIDS[name]
    seen = {}
    for i, tg in enumerate(tags):
        if tg[0] in ("lo", "hi"):
            seen[(tg[0], tg[1], tg[3])] = int(cell[i])
        if tg[0] == "time" and tg[1] == -1 and tg[4] == 0:
            seen[("time", tg[2], tg[3])] = int(cell[i])
    for a in range(3):
        n = BC.axis(grid, a)[2]
        if a < 2 or BC.heights(BC.axis(grid, a)[0])[0]:
            assert seen[("lo", a, 0)] >= 0 and BC.decompose(grid, seen[("lo", a, 0)])[a] == 0      # lower bounds inclusive
        assert seen[("lo", a, -1)] == -1                                                           # one double below: out
        if a < 2 or BC.heights(BC.axis(grid, a)[1])[0]:
            assert seen[("hi", a, 0)] == -1                                                        # upper bounds exclusive
        # one double below the upper bound: the last cell, or the guard
        last = seen[("hi", a, -1)]
        assert (last >= 0 and BC.decompose(grid, last)[a] == n - 1) or facts["guard_decides"][BC.AXES[a]] >= 1
        # the last cell holds a placed particle in any case
        assert any(c >= 0 and BC.decompose(grid, int(c))[a] == n - 1 for c in cell[:npl])
    # time < t0 and time > t1 are outside; both ends belong to the window
    assert seen[("time", 0, -1)] == -1 and seen[("time", 0, 0)] >= 0 and seen[("time", 0, 1)] >= 0
    assert seen[("time", 1, -1)] >= 0 and seen[("time", 1, 0)] >= 0 and seen[("time", 1, 1)] == -1
    assert seen[("time", 2, 0)] >= 0
    on_faces = [int(cell[i]) >= 0 for i, tg in enumerate(tags) if tg[0] == "time" and tg[1] >= 0]
    assert any(on_faces) and not all(on_faces)


def test_cells_either_side_of_every_placed_face_are_occupied(case):
    name, atm, npl, tags, facts, cell = case
    grid = BC.GRIDS[name]
    count = 0
    for which in (0, 1):
        for a in range(3):
            n = BC.axis(grid, a)[2]
            line = {}
            for i, tg in enumerate(tags):
                if tg[0] == "face" and tg[1] == a and tg[4] == which and cell[i] >= 0:
                    line.setdefault(BC.decompose(grid, int(cell[i]))[a], []).append(i)
            for k in BC.face_numbers(grid, a, BC.EVERY[name]):
                for c in (k - 1, k):
                    if 0 <= c < n:
                        assert c in line, (name, a, k, c)
                        count += 1
    print("BOX_CASE " + json.dumps({"grid": name, "occupied_cells_beside_faces": count}))


def test_heights_on_the_faces(case):
    """At least half of the placed z faces have a pressure whose Z is the face to the bit, and every face is bracketed
    by the Z of two pressures."""
    name, _, _, _, facts, _ = case
    exact, n = facts["exact_heights"]
    assert 2 * exact >= n and facts["bracketed"] == n, facts
    grid = BC.GRIDS[name]
    for k in BC.face_numbers(grid, 2, BC.EVERY[name]):
        z = BC.face(grid, 2, k)
        ex, below, above = BC.heights(z)
        assert BC.Z(below) < z < BC.Z(above) and all(BC.Z(p) == z for p in ex)


def _libm_Z(p):
    return np.array([RA.Z(v) for v in np.asarray(p, dtype=np.float64).tolist()])


@pytest.mark.parametrize("nens", [0, BC.NMEMBER])
def test_oracle_mixing_equals_the_numpy_restatement(nens, monkeypatch):
    """module_mixing of the oracle against tests/refmodules.py on grid A, bit for bit (the restatement with the C
    library's logarithm; with members it mixes each member's particles on their own, in index order)."""
    monkeypatch.setattr(RM, "Z", _libm_Z)
    ctl, clim, m0, m1 = BC.setup("A", nens)
    atm, npl, tags = BC.particles("A", T, DT)
    o = B.Oracle(ctl, clim, m0, m1, atm)
    ref = RM.Ref(o.ctl, clim, m0, m1)
    before = o.q.copy()
    o.module("mixing", T)
    want = before.copy()
    groups = [np.nonzero(atm["q"][BC.QENS] == e)[0] for e in range(nens)] if nens else [np.arange(len(atm["time"]))]
    for g in groups:
        rows = ref.mixing(T, atm["time"][g], atm["lon"][g], atm["lat"][g], atm["p"][g],
                          [before[k][g] for k in (BC.QM, BC.QVMR, BC.QAOA)])
        for k, row in zip((BC.QM, BC.QVMR, BC.QAOA), rows):
            want[k][g] = row
    assert np.array_equal(o.q, want)
    cell = BC.cells(BC.GRIDS["A"], atm, T, DT)
    assert np.array_equal(o.q[:, cell < 0], before[:, cell < 0])
    changed = np.count_nonzero(o.q[BC.QM][:npl] != before[BC.QM][:npl])
    print("BOX_CASE " + json.dumps({"grid": "A", "nens": nens, "placed_mixed": int(changed)}))
    assert changed > np.count_nonzero(cell[:npl] >= 0) // 2      # (with members: only beside a particle of its own member)


def test_oracle_grid_sums_equal_the_box_sums(case):
    """Oracle.grid_sums and refanalysis.box_sums where the two definitions coincide (one member, no weighting function):
    the same sums of every quantity, the same cells."""
    name, atm, npl, tags, facts, cell = case
    ctl, clim, m0, m1 = BC.setup(name)
    o = B.Oracle(ctl, clim, m0, m1, atm)
    cnt, mean, _ = o.grid_sums(T)
    assert np.array_equal(cnt, np.bincount(cell[cell >= 0], minlength=len(cnt)))
    for k in (BC.QM, BC.QAOA):
        assert np.array_equal(mean[k], RA.box_sums(atm, BC.GRIDS[name], T, DT, k)[0])
    assert cnt.sum() >= facts["inside"] > 0
