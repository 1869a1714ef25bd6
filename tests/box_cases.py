"""Edge inputs of the box arithmetic: particles on cell faces, on the bounds of the box and on the ends of the time window.

Six device consumers decide a particle's box the same way (box_cell, box_cell_of_height, ground_cell in
mptrac_amd/csrc/mphip_kernels.hpp; the reference: mptrac.c:5201-5218, 13836-13855, output.c's box_column / box_cell):

  inside : !(time < t0 || time > t1 || lon < lon0 || lon >= lon1 || lat < lat0 || lat >= lat1 || z < z0 || z >= z1)
  index  : ix = (int) ((lon - lon0) / dlon), dlon = (lon1 - lon0) / nx        (same for lat and z = Z(p))
  guard  : ix >= nx || iy >= ny || iz >= nz -> outside

  GRIDS       boxes with inexact cell widths, longitudes beyond 180, a latitude box wider than the globe, the default
              mixing grid and a tiny window
  placed      a particle on every face of every axis (lo + k d as the kernel's arithmetic gives it), one double either
              side, the two doubles either side of the border the truncated quotient draws (threshold: on an inexact
              width, or at lon = 0 on the default grid, that border is not next to lo + k d), the corners, the bounds,
              the ends of the time window, and light neighbours of every member in the cells beside each face
  heights     for a height, pressures whose Z (the C library's log) is that height, or brackets it
  particles   the placed particles in front of a random background; the placed ones carry 1000 times the background's
              quantity values, so one of them in the wrong cell moves a cell's mean and sum by far more than any bar
  weighting   a vertical weighting function with nodes that are Z of placed pressures
  facts       what the inputs do, from the reference arithmetic alone (tests/test_box_edges_cpu.py asserts them)
"""
import math

import numpy as np

import refanalysis as RA

H0, P0 = RA.H0, RA.P0
Z = RA.Z

# (lon0, lon1, nx, lat0, lat1, ny, z0, z1, nz), the order of refanalysis.box_cell and Simulation.box_sums
GRIDS = {
    "A": (-180.0, 180.0, 7, -90.0, 90.0, 11, 2.0, 25.0, 9),          # every width inexact
    "B": (0.0, 360.0, 49, -43.0, 127.0, 17, 0.0, 24.0, 7),           # beyond 180 degrees, wider than the globe
    "C": (-180.0, 180.0, 360, -90.0, 90.0, 180, -5.0, 85.0, 90),     # the reference's default mixing grid
    "D": (10.0, 10.5, 3, 20.0, 20.2, 2, 5.0, 6.0, 4),                # a tiny window
}
EVERY = {"A": 1, "B": 1, "C": 30, "D": 1}      # which faces are placed
AXES = ("lon", "lat", "z")
NAMES = ("m", "vmr", "aoa", "ens")             # the first three are mixed by module_mixing
QM, QVMR, QAOA, QENS = 0, 1, 2, 3
NMEMBER = 3
HEAVY = 1e3                                     # placed / background quantity values
N_BACKGROUND = 2000
SEARCH = 40                                     # doubles either side of P0 exp(-z / H0) looked at for Z(p) == z


T, DT_MOD = 360.0, 180.0                       # the window [270, 450]: its ends and its middle are exact
MET_GRID = (36, 19, 40)


def grid_keys(prefix, grid):
    lon0, lon1, nx, lat0, lat1, ny, z0, z1, nz = grid
    return {prefix + "_lon0": lon0, prefix + "_lon1": lon1, prefix + "_nx": nx, prefix + "_lat0": lat0,
            prefix + "_lat1": lat1, prefix + "_ny": ny, prefix + "_z0": z0, prefix + "_z1": z1, prefix + "_nz": nz}


def setup(name, nens=0, **over):
    """(ctl, clim, met0, met1) with grid `name` as the mixing grid and the output grid; module_mixing is not due in a
    time step before t = 3600, so a step at the first particle time only stores the particles"""
    import cases
    from mptrac_amd.ctl import ctl_from_quantities
    from mptrac_amd.synth import synthetic_met
    ctl = dict(cases.BASE, mixing_trop=0.4, mixing_strat=0.1, mixing_dt=3600.0, nens=nens, **ctl_from_quantities(NAMES))
    ctl.update(grid_keys("mixing", GRIDS[name]))
    ctl.update(grid_keys("grid", GRIDS[name]))
    ctl.update(over)
    m0 = synthetic_met(MET_GRID, 0.0, 1.0, fields=cases.PRESSURE_LEVEL_FIELDS)
    m1 = synthetic_met(MET_GRID, 3600.0, 1.25, fields=cases.PRESSURE_LEVEL_FIELDS)
    return ctl, cases.load_clim_tropo(), m0, m1


def axis(grid, a):
    """(lo, hi, n) of axis a = 0, 1, 2"""
    return grid[3 * a], grid[3 * a + 1], grid[3 * a + 2]


def width(grid, a):
    lo, hi, n = axis(grid, a)
    return (hi - lo) / n


def face(grid, a, k):
    """fl(lo + k d): the face's coordinate from the kernel's own cell width"""
    lo, _, _ = axis(grid, a)
    return lo + k * width(grid, a)


def quotient(grid, a, x):
    lo, _, _ = axis(grid, a)
    return (x - lo) / width(grid, a)


def index(grid, a, x):
    """the cell index of coordinate x along axis a, -1 outside (bounds, then the guard)"""
    lo, hi, n = axis(grid, a)
    if x < lo or x >= hi:
        return -1
    i = int(quotient(grid, a, x))
    return -1 if i >= n else i


def face_numbers(grid, a, every=1):
    n = axis(grid, a)[2]
    ks = list(range(0, n + 1, every))
    if ks[-1] != n:
        ks.append(n)
    return ks


def heights(z):
    """Pressures around P0 exp(-z / H0): (exact, below, above) -- the pressures with Z(p) == z, the pressure with the
    largest Z < z and the one with the smallest Z > z among the 2 SEARCH + 1 doubles looked at (None: not found)."""
    cand = _scan(z)
    exact = sorted(q for q in cand if Z(q) == z)
    under = [q for q in cand if Z(q) < z]
    over = [q for q in cand if Z(q) > z]
    below = max(under, key=Z) if under else None        # (Z falls with p: the smallest such p)
    above = min(over, key=Z) if over else None
    return exact, below, above


def _scan(z):
    p = P0 * math.exp(-z / H0)
    cand = [p]
    lo = hi = p
    for _ in range(SEARCH):
        lo, hi = math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf)
        cand += [lo, hi]
    return sorted(cand)


def threshold(grid, a, k):
    """The two neighbouring doubles between which the truncated quotient reaches k -- where the arithmetic itself puts the
    border of cell k, which on an axis with an inexact width is not always within one double of lo + k d: [(coordinate,
    side)] with side -2 below the border and +2 on it (pressures on the z axis; [] if the border is not found nearby)."""
    lo, _, _ = axis(grid, a)
    d = width(grid, a)

    def reached(x):
        return int((x - lo) / d) >= k

    if a == 2:
        cand = _scan(face(grid, a, k))[::-1]      # ascending Z
        for p_lo, p_hi in zip(cand, cand[1:]):
            if not reached(Z(p_lo)) and reached(Z(p_hi)):
                return [(p_lo, -2), (p_hi, 2)]
        return []
    lower, upper = face(grid, a, k) - 0.5 * d, face(grid, a, k) + 0.5 * d      # bisection over the doubles
    if reached(lower) or not reached(upper):
        return []
    while True:
        mid = lower + 0.5 * (upper - lower)
        if not lower < mid < upper:
            break
        if reached(mid):
            upper = mid
        else:
            lower = mid
    assert math.nextafter(lower, math.inf) == upper
    return [(lower, -2), (upper, 2)]


def points(grid, a, x, k=None):
    """[(coordinate, side)] for the value x of axis a: the value itself (side 0), the double below (-1) and above (+1);
    on the z axis the coordinate is a pressure and the sides are those of Z(p) (an exact pressure only if one exists).
    With the face number k > 0 also the two doubles either side of the border the arithmetic draws (threshold)."""
    if a < 2:
        out = [(x, 0), (math.nextafter(x, -math.inf), -1), (math.nextafter(x, math.inf), 1)]
    else:
        exact, below, above = heights(x)
        out = [(exact[0], 0)] if exact else []
        if below is not None:
            out.append((below, -1))
        if above is not None:
            out.append((above, 1))
    if k:
        have = {c for c, _ in out}
        out += [(c, s) for c, s in threshold(grid, a, k) if c not in have]
    return out


def generic(grid, which):
    """(lon, lat, p) well inside a cell on every axis; which = 1: the centre of another cell"""
    out = []
    for a in range(3):
        lo, hi, n = axis(grid, a)
        d = width(grid, a)
        x = lo + (int(0.37 * n) + 0.3) * d if which == 0 else lo + (int(0.71 * n) + 0.5) * d
        out.append(x if a < 2 else P0 * math.exp(-x / H0))
    return out


def placed(grid, t, dt_mod, every=1, times="all"):
    """lon, lat, p, time and a tag per placed particle.  tag = (kind, axis, k, side, which):
    kind "face" (face k of the axis; side 0: on lo + k d, -1 / +1: the double below / above, -2 / +2: the doubles below /
    on the border the arithmetic draws), "hi" / "lo" (a bound of the box; side 0 or -1), "mate" (a light particle in the
    middle of cell k of the axis, side = its member), "corner", "time" (k = 0: the lower end of the window, 1: the upper
    end, 2: t itself; axis -1: at a generic position, else on a face of that axis).  `which`: the generic position of
    the other coordinates.  times = "late": only times >= t (a particle released at t or later takes no step at t)."""
    rows = []

    def put(a, coord, tag, which, time=t):
        pos = generic(grid, which)
        pos[a] = coord
        rows.append((pos[0], pos[1], pos[2], time, tag + (which,)))

    for a in range(3):
        lo, hi, n = axis(grid, a)
        for k in face_numbers(grid, a, every):
            for coord, side in points(grid, a, face(grid, a, k), k):
                for which in (0, 1):
                    put(a, coord, ("face", a, k, side), which)
        for kind, bound in (("hi", hi), ("lo", lo)):
            for coord, side in points(grid, a, bound):
                if side <= 0:
                    put(a, coord, (kind, a, n if kind == "hi" else 0, side), 0)
    # a light particle of every member in the middle of each cell either side of a placed face, along both lines: a
    # placed particle has a neighbour of its own member wherever the arithmetic puts it
    for a in range(3):
        lo, hi, n = axis(grid, a)
        wanted = sorted({c for k in face_numbers(grid, a, every) for c in (k - 1, k) if 0 <= c < n})
        for c in wanted:
            x = lo + (c + 0.5) * width(grid, a)
            for which in (0, 1):
                for member in range(NMEMBER):
                    put(a, x if a < 2 else P0 * math.exp(-x / H0), ("mate", a, c, member), which)
    # corners: of the box, and of the cell of the first generic position
    for ks in ([(0, axis(grid, a)[2]) for a in range(3)], [(int(0.37 * axis(grid, a)[2]),) * 2 for a in range(3)]):
        ks = [(k0, k1 if k1 != k0 else k0 + 1) for k0, k1 in ks]
        for i in ks[0]:
            for j in ks[1]:
                for l in ks[2]:
                    pz = points(grid, 2, face(grid, 2, l))
                    rows.append((face(grid, 0, i), face(grid, 1, j), pz[0][0], t, ("corner", -1, (i, j, l), pz[0][1], 0)))
    # the time window
    t0, t1 = t - 0.5 * dt_mod, t + 0.5 * dt_mod
    stamps = [(0, s, v) for v, s in points(grid, 0, t0)] + [(1, s, v) for v, s in points(grid, 0, t1)] + [(2, 0, t)]
    if times == "late":
        stamps = [st for st in stamps if st[2] >= t]
    for end, side, v in stamps:
        for which in (0, 1):
            pos = generic(grid, which)
            rows.append((pos[0], pos[1], pos[2], v, ("time", -1, end, side, which)))
        for a in range(3):
            k = min(1, axis(grid, a)[2] - 1) if a != 1 else axis(grid, a)[2] // 2
            pts = points(grid, a, face(grid, a, k))
            coord = pts[0][0] if a != 1 else pts[1][0]
            put(a, coord, ("time", a, end, side), 0, time=v)
    lon, lat, p, time, tags = (list(c) for c in zip(*rows))
    return {"lon": np.array(lon), "lat": np.array(lat), "p": np.array(p), "time": np.array(time), "tag": tags}


def particles(name, t, dt_mod, seed=7, times="all", n_background=N_BACKGROUND):
    """(atm, number placed, tags): the placed particles of grid `name` first, then a random background inside and around
    the box, a tenth of it outside the time window.  Quantities NAMES; the placed ones HEAVY times the background's, all
    different (the "mate" particles keep the background's scale); ens = index mod NMEMBER (round robin over the placed
    particles), a mate's own member."""
    grid = GRIDS[name]
    pl = placed(grid, t, dt_mod, EVERY[name], times)
    npl = len(pl["tag"])
    rng = np.random.default_rng(seed)
    n = npl + n_background
    atm = {}
    cols = []
    for a in range(3):
        lo, hi, _ = axis(grid, a)
        cols.append(rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), n_background))
    cols[1] = np.clip(cols[1], -90.0, 90.0)
    atm["lon"] = np.concatenate([pl["lon"], cols[0]])
    atm["lat"] = np.concatenate([pl["lat"], cols[1]])
    atm["p"] = np.concatenate([pl["p"], P0 * np.exp(-cols[2] / H0)])
    tb = np.full(n_background, float(t))
    tb[::10] = t - dt_mod
    atm["time"] = np.concatenate([pl["time"], tb])
    mate = np.array([tg[0] == "mate" for tg in pl["tag"]] + [False] * n_background)
    scale = np.where((np.arange(n) < npl) & ~mate, HEAVY, 1.0)
    q = np.zeros((len(NAMES), n))
    q[QM] = scale * (0.5 + rng.random(n))
    q[QVMR] = scale * 1e-9 * (1.0 + rng.random(n))
    q[QAOA] = scale * (1.0 + rng.random(n))
    q[QENS] = np.arange(n) % NMEMBER
    for i, tg in enumerate(pl["tag"]):
        if tg[0] == "mate":
            q[QENS][i] = tg[3]
    atm["q"] = q
    for k in ("lon", "lat", "p", "time"):
        atm[k] = np.ascontiguousarray(atm[k], dtype=np.float64)
        assert np.all(np.isfinite(atm[k]))
    return atm, npl, pl["tag"]


def weighting(name, atm, tags):
    """(kz, kw), indices of the nodes that are Z of a placed pressure: nodes on up to three placed z faces (a particle sits
    exactly on the first, on the last and, with three, on an inner node), one node between the first two; faces of the
    box lie below the first and above the last node."""
    fz = face_numbers(GRIDS[name], 2, EVERY[name])
    ks = sorted({fz[1], fz[len(fz) // 2], fz[-2]})
    assert len(ks) >= 2 and 0 < ks[0] and ks[-1] < fz[-1], ks
    kz = []
    for k in ks:
        ip = [i for i, tg in enumerate(tags) if tg[0] == "face" and tg[1] == 2 and tg[2] == k]
        kz.append(Z(float(atm["p"][ip[0]])))
    kz.insert(1, 0.5 * (kz[0] + kz[1]))
    assert all(b > a for a, b in zip(kz, kz[1:]))
    return (np.array(kz), np.array([0.2, 1.0, 0.6, 0.1][:len(kz)])), [0] + list(range(2, len(kz)))


def cells(grid, atm, t, dt_mod):
    """the reference's cell of every particle (refanalysis.box_cell behind the time window), -1 outside"""
    t0, t1 = t - 0.5 * dt_mod, t + 0.5 * dt_mod
    out = np.full(len(atm["time"]), -1, dtype=np.int64)
    for i, (tp, lon, lat, p) in enumerate(zip(atm["time"].tolist(), atm["lon"].tolist(), atm["lat"].tolist(),
                                              atm["p"].tolist())):
        if not (tp < t0 or tp > t1):
            out[i] = RA.box_cell(grid, lon, lat, Z(p))
    return out


def coordinate(atm, a, i):
    return float(atm[AXES[a] if a < 2 else "p"][i]) if a < 2 else Z(float(atm["p"][i]))


def facts(name, atm, tags, t, dt_mod):
    """What the inputs of grid `name` do, from the reference arithmetic alone."""
    grid = GRIDS[name]
    cell = cells(grid, atm, t, dt_mod)
    f = {"grid": name, "placed": len(tags), "inside": int(np.count_nonzero(cell[:len(tags)] >= 0))}
    # a face's own point in cell k - 1; the guard decides below the upper bound
    f["face_in_lower_cell"], f["below_in_upper_cell"], f["guard_decides"] = {}, {}, {}
    for a in range(3):
        lo, hi, n = axis(grid, a)
        low = [k for k in range(1, n) if index(grid, a, face(grid, a, k)) == k - 1]
        f["face_in_lower_cell"][AXES[a]] = (len(low), n)
        up = [k for k in range(1, n) if a < 2 and index(grid, a, math.nextafter(face(grid, a, k), -math.inf)) == k]
        f["below_in_upper_cell"][AXES[a]] = (len(up), n)
        guard = 0
        for i, tg in enumerate(tags):
            if tg[0] in ("face", "hi") and tg[1] == a:
                x = coordinate(atm, a, i)
                if x < hi and quotient(grid, a, x) == n:
                    guard += 1
                    assert cell[i] == -1
        f["guard_decides"][AXES[a]] = guard
    ks = face_numbers(grid, 2, EVERY[name])
    found = [heights(face(grid, 2, k)) for k in ks]
    f["exact_heights"] = (sum(1 for e, _, _ in found if e), len(ks))
    f["bracketed"] = sum(1 for _, b, a_ in found if b is not None and a_ is not None)
    return f, cell


def decompose(grid, c):
    ny, nz = grid[5], grid[8]
    return c // (ny * nz), (c // nz) % ny, c % nz


def flip_effects(grid, cell, values, mixparam, tags, nens=0, ens=None):
    """For every placed particle on or beside a face (generic in the other two coordinates): the largest relative change
    of any particle's value after module_mixing if that one particle were in the cell on the other side of its face
    instead (outside, beyond the box).  values: one mixed quantity; mixparam: per particle.  Returns the smallest of
    these over the particles -- the margin a tolerance must stay below."""
    nx, ny, nz = grid[2], grid[5], grid[8]
    ngrid = nx * ny * nz
    full = np.where(cell >= 0, cell + (ens.astype(np.int64) * ngrid if nens else 0), -1)
    members = {}
    for i, c in enumerate(full.tolist()):
        if c >= 0:
            members.setdefault(c, []).append(i)

    def after(idx):
        if not idx:
            return {}
        mean = sum(values[i] for i in idx) / len(idx)
        return {i: values[i] + (mean - values[i]) * mixparam[i] for i in idx}

    worst, n = math.inf, 0
    stride = (ny * nz, nz, 1)
    for i, tg in enumerate(tags):
        if tg[0] != "face":
            continue
        a, k = tg[1], tg[2]
        c = int(cell[i])
        if c < 0:       # (outside: its neighbours inside are looked at from their side)
            continue
        off = int(ens[i]) * ngrid if nens else 0
        here = decompose(grid, c)[a]
        there = here - 1 if here == k else here + 1        # across face k
        other = c + (there - here) * stride[a] + off if 0 <= there < grid[3 * a + 2] else -1
        c += off
        old = dict(after(members.get(c, [])))
        old.update(after(members.get(other, [])) if other >= 0 else {})
        new = dict(after([j for j in members.get(c, []) if j != i]))
        if other >= 0:
            new.update(after(members.get(other, []) + [i]))
        else:
            new[i] = values[i]
        change = max(abs(new[j] - old[j]) / abs(old[j]) for j in old)
        worst = min(worst, change)
        n += 1
    return worst, n
