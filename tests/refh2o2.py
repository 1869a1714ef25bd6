"""Scalar restatement of module_chem_grid and module_h2o2_chem, for the SO2 chemistry tests.

module_chem_grid: the chemistry grid (CHEMGRID_*) has nz levels of height dz between z0 and z1 (Z(p) = H0 log(P0 / p)),
nx x ny cells between lon0 / lon1 and lat0 / lat1.  A particle is in a cell if its time lies in [t - DT_MOD / 2,
t + DT_MOD / 2] and lon0 <= lon < lon1, lat0 <= lat < lat1, z0 <= Z(p) < z1 (the bounds are tested before the indices are
truncated, as module_mixing's box_cell does); with an ensemble (NENS > 0) the cell lies in the copy of the grid of its
member, cell + ens * ngrid.  The masses q[m] of each cell are summed in particle-index order (np.add.at); every particle in
a cell then gets Cx = MA / MOLMASS * mass / (1e9 RHO(press, temp) area dz), with press, lon, lat the cell centre, area
the cell's area and temp the temperature at the cell centre at the step time t (intpol_met_time_3d).  Particles outside
keep their Cx.

module_h2o2_chem: every particle with dt != 0 inside a cloud (lwc > 0 or rwc > 0 at the particle) loses the fraction
1 - exp(-dt rate) of m and vmr, with the rate of the aqueous-phase oxidation of SO2 by H2O2 (rate() below).

Two arithmetic modes as in tests/refchem.py: "numpy" and "libm" (exp, pow, cos, log of the C library through ctypes; the
reference-rounding build's yardstick).  The temperature, lwc, rwc and H2O2 at the particle come from the oracle's
module_meteo, the cell-centre temperature from orc_intpol_met_time_3d."""
import ctypes as C
import math

import numpy as np

AVO = 6.02214e23
RI = 8.3144598
MA = 28.9644
RA = 1e3 * RI / MA
RE = 6367.421
P0 = 1013.25
H0 = 7.0
COR_A = 3.12541941e-06
COR_B = -5.72532259e-01

_libm = None


def _lib():
    global _libm
    if _libm is None:
        _libm = C.CDLL("libm.so.6")
        for f in ("exp", "cos", "log"):
            getattr(_libm, f).restype = C.c_double
            getattr(_libm, f).argtypes = [C.c_double]
        _libm.pow.restype = C.c_double
        _libm.pow.argtypes = [C.c_double, C.c_double]
    return _libm


def _funcs(mode):
    if mode == "libm":
        L = _lib()
        return L.exp, L.pow, L.cos, L.log
    return ((lambda x: float(np.exp(x))), (lambda x, y: float(np.power(x, y))), (lambda x: float(np.cos(x))),
            (lambda x: float(np.log(x))))


def low():
    """the threshold of the high-SO2 correction, pow(1 / a, 1 / b) of the C library"""
    return _lib().pow(1. / COR_A, 1. / COR_B)


# ---- module_chem_grid ---------------------------------------------------------------------------------------------

def grid_tables(ctl, mode="numpy"):
    """(press[nz], lon[nx], lat[ny], area[ny], dz) of the chemistry grid; ctl: dict with the chemgrid_* keys"""
    exp, _, cos, _ = _funcs(mode)
    nx, ny, nz = ctl["chemgrid_nx"], ctl["chemgrid_ny"], ctl["chemgrid_nz"]
    dz = (ctl["chemgrid_z1"] - ctl["chemgrid_z0"]) / nz
    dlon = (ctl["chemgrid_lon1"] - ctl["chemgrid_lon0"]) / nx
    dlat = (ctl["chemgrid_lat1"] - ctl["chemgrid_lat0"]) / ny
    press = np.array([P0 * exp(-(ctl["chemgrid_z0"] + dz * (iz + 0.5)) / H0) for iz in range(nz)])
    lon = np.array([ctl["chemgrid_lon0"] + dlon * (ix + 0.5) for ix in range(nx)])
    lat = np.array([ctl["chemgrid_lat0"] + dlat * (iy + 0.5) for iy in range(ny)])
    area = np.array([dlat * dlon * ((RE * math.pi / 180.) * (RE * math.pi / 180.)) * cos(lat[iy] * math.pi / 180.)
                     for iy in range(ny)])
    return press, lon, lat, area, dz


def cells(ctl, t, time, p, lon, lat, ens=None, mode="numpy"):
    """cell of every particle (ix, iy, iz, flat index with the ensemble offset), -1 outside"""
    log = _funcs(mode)[3]
    nx, ny, nz = ctl["chemgrid_nx"], ctl["chemgrid_ny"], ctl["chemgrid_nz"]
    dz = (ctl["chemgrid_z1"] - ctl["chemgrid_z0"]) / nz
    dlon = (ctl["chemgrid_lon1"] - ctl["chemgrid_lon0"]) / nx
    dlat = (ctl["chemgrid_lat1"] - ctl["chemgrid_lat0"]) / ny
    t0, t1 = t - 0.5 * ctl["dt_mod"], t + 0.5 * ctl["dt_mod"]
    n = len(time)
    out = np.full(n, -1, dtype=np.int64)
    ixs, iys, izs = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for i in range(n):
        z = H0 * log(P0 / p[i])
        if (time[i] < t0 or time[i] > t1 or lon[i] < ctl["chemgrid_lon0"] or lon[i] >= ctl["chemgrid_lon1"]
                or lat[i] < ctl["chemgrid_lat0"] or lat[i] >= ctl["chemgrid_lat1"] or z < ctl["chemgrid_z0"]
                or z >= ctl["chemgrid_z1"]):
            continue
        ix = int((lon[i] - ctl["chemgrid_lon0"]) / dlon)
        iy = int((lat[i] - ctl["chemgrid_lat0"]) / dlat)
        iz = int((z - ctl["chemgrid_z0"]) / dz)
        if ix >= nx or iy >= ny or iz >= nz:
            continue
        ixs[i], iys[i], izs[i] = ix, iy, iz
        out[i] = (ix * ny + iy) * nz + iz + (int(ens[i]) * nx * ny * nz if ens is not None else 0)
    return out, ixs, iys, izs


def chem_grid(ctl, q, idx, t, time, p, lon, lat, temp_at, mode="numpy"):
    """module_chem_grid on the quantity rows q in place; idx: qnt indices m, Cx, ens (-1 = absent).
    temp_at(t, press, lon, lat) -> temperature at one point.  Returns (cell, mass per cell)."""
    if idx.get("m", -1) < 0 or idx.get("Cx", -1) < 0:
        return None, None
    nx, ny, nz = ctl["chemgrid_nx"], ctl["chemgrid_ny"], ctl["chemgrid_nz"]
    ngrid = nx * ny * nz
    nens = ctl.get("nens", 0)
    ens = q[idx["ens"]] if nens > 0 and idx.get("ens", -1) >= 0 else None
    press, glon, glat, area, dz = grid_tables(ctl, mode)
    cell, ixs, iys, izs = cells(ctl, t, time, p, lon, lat, ens, mode)
    ok = cell >= 0
    mass = np.zeros(ngrid * (nens if nens > 0 else 1))
    np.add.at(mass, cell[ok], q[idx["m"]][ok])
    value = {}
    for i in np.nonzero(ok)[0]:
        c = int(cell[i])
        if c not in value:
            pr = press[izs[i]]
            temp = temp_at(t, pr, glon[ixs[i]], glat[iys[i]])
            rho = 100. * pr / (RA * temp)
            value[c] = MA / ctl["molmass"] * mass[c] / (1e9 * rho * area[iys[i]] * dz)
        q[idx["Cx"], i] = value[c]
    return cell, mass


# ---- module_h2o2_chem ---------------------------------------------------------------------------------------------

def rate(p, t, lwc, rwc, h2o2_zm, cx, mode="numpy"):
    """rate coefficient of one particle in a cloud: pressure p [hPa], temperature t [K], lwc, rwc [kg/kg], the H2O2
    zonal mean at the particle, its Cx (None: the particle carries no Cx)"""
    exp, pw, _, _ = _funcs(mode)
    M = AVO * 1e-6 * (p * 100) / (RI * t)
    k = 9.1e7 * exp(-29700 / RI * (1. / t - 1. / 298.15))
    H_SO2 = 1.3e-2 * exp(2900 * (1. / t - 1. / 298.15)) * RI * t
    K_1S = 1.23e-2 * exp(2.01e3 * (1. / t - 1. / 298.15))
    H_h2o2 = 8.3e2 * exp(7600 * (1 / t - 1 / 298.15)) * RI * t
    cor = 1.
    if cx is not None:
        cor = COR_A * pw(cx, COR_B) if cx > low() else 1
    h2o2 = H_h2o2 * h2o2_zm * M * cor * 1000. / AVO
    rho_air = p / (RI * t) * MA / 10.
    CWC = (lwc + rwc) * rho_air / 1e3
    return k * K_1S * h2o2 * H_SO2 * CWC


def h2o2_chem(q, idx, p, t, lwc, rwc, h2o2_zm, dt, mode="numpy"):
    """module_h2o2_chem on the quantity rows q in place; idx: m, vmr, mloss_h2o2, loss_rate, Cx (-1 = absent)."""
    exp = _funcs(mode)[0]
    for i in range(q.shape[1]):
        if dt[i] == 0:
            continue
        if not (lwc[i] > 0 or rwc[i] > 0):
            continue
        cx = float(q[idx["Cx"], i]) if idx.get("Cx", -1) >= 0 else None
        r = rate(float(p[i]), float(t[i]), float(lwc[i]), float(rwc[i]), float(h2o2_zm[i]), cx, mode)
        aux = exp(-float(dt[i]) * r)
        if idx.get("m", -1) >= 0:
            m = q[idx["m"], i]
            if idx.get("mloss_h2o2", -1) >= 0:
                q[idx["mloss_h2o2"], i] += m * (1 - aux)
            q[idx["m"], i] = m * aux
            if idx.get("loss_rate", -1) >= 0:
                q[idx["loss_rate"], i] += r
        if idx.get("vmr", -1) >= 0:
            q[idx["vmr"], i] *= aux
    return q
