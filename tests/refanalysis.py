"""Reference of the device's analysis outputs (mphip_box_sums, mphip_sample_obs, mphip_station_hits): the particle
loops of write_csi / write_prof, write_sample and write_station of mptrac_amd/host/output.c, transcribed line by line.

cos, sin, log and exp are the C library's (Python's math module calls libm; numpy's vector functions are not glibc's and
are not used for them).  Plain +, -, *, / of Python floats and numpy float64 arrays are IEEE operations, one rounding each,
in the order written -- so the membership decisions and, with sums added one particle after the other, the sums are the
host loop's bits."""
import math

import numpy as np

RE, H0, P0 = 6367.421, 7.0, 1013.25


def _libm(f, x, at_zero=math.nan):
    """f(x) of the C library where Python's math module raises instead: cos / sin of an infinity and the logarithm of a
    negative number are NaN, log(+-0) is -inf.  Every other argument goes through math's call of libm unchanged."""
    try:
        return f(x)
    except ValueError:
        return at_zero if x == 0 else math.nan


def Z(p):
    return H0 * _libm(math.log, P0 / p, -math.inf)


def P(z):
    return P0 * math.exp(-z / H0)


def geo2cart(z, lon, lat):
    r, phi, lam = RE + z, lat * (math.pi / 180.0), lon * (math.pi / 180.0)
    cos_phi, sin_phi, cos_lam, sin_lam = _libm(math.cos, phi), _libm(math.sin, phi), _libm(math.cos, lam), _libm(math.sin, lam)
    return (r * cos_phi * cos_lam, r * cos_phi * sin_lam, r * sin_phi)


def kernel_weight(kz, kw, p):
    nk = len(kz)
    if nk < 2:
        return 1.0
    z = Z(p)
    if z < kz[0]:
        return kw[0]
    if z > kz[nk - 1]:
        return kw[nk - 1]
    lo, hi = 0, nk - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if kz[mid] > z:
            hi = mid
        else:
            lo = mid
    # (C's division: a repeated node gives +-inf or NaN where Python's / raises; the same bits everywhere else)
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = float(np.float64(kw[lo + 1] - kw[lo]) / np.float64(kz[lo + 1] - kz[lo]))
    return kw[lo] + slope * (z - kz[lo])


def box_cell(box, lon, lat, z):
    """box_column + box_cell; box = (lon0, lon1, nx, lat0, lat1, ny, z0, z1, nz)"""
    lon0, lon1, nx, lat0, lat1, ny, z0, z1, nz = box
    dlon, dlat, dz = (lon1 - lon0) / nx, (lat1 - lat0) / ny, (z1 - z0) / nz
    if lon < lon0 or lon >= lon1 or lat < lat0 or lat >= lat1:
        return -1
    ix, iy = int((lon - lon0) / dlon), int((lat - lat0) / dlat)
    if ix >= nx or iy >= ny:
        return -1
    if z < z0 or z >= z1:
        return -1
    iz = int((z - z0) / dz)
    if iz >= nz:
        return -1
    return (ix * ny + iy) * nz + iz


class MemberOutOfRange(Exception):
    pass


def box_sums(atm, box, t, dt_mod, qnt, nmember=1, qnt_member=-1, kernel=((), ())):
    """the loops output.c:377-387 (CSI) and 557-563 (profiles): sum[member][cell]"""
    kz, kw = [float(v) for v in kernel[0]], [float(v) for v in kernel[1]]
    t0, t1 = t - 0.5 * dt_mod, t + 0.5 * dt_mod
    ncell = box[2] * box[5] * box[8]
    out = [0.0] * (nmember * ncell)
    time, p, lon, lat, q = atm["time"].tolist(), atm["p"].tolist(), atm["lon"].tolist(), atm["lat"].tolist(), atm["q"]
    val = q[qnt].tolist()
    mem = q[qnt_member].tolist() if qnt_member >= 0 else None
    for ip in range(len(time)):
        if time[ip] < t0 or time[ip] > t1:
            continue
        member = int(mem[ip]) if mem is not None else 0
        if member < 0 or member >= nmember:
            raise MemberOutOfRange(ip)
        c = box_cell(box, lon[ip], lat[ip], Z(p[ip]))
        if c >= 0:
            out[member * ncell + c] += kernel_weight(kz, kw, p[ip]) * val[ip]
    return np.array(out).reshape(nmember, ncell)


def cartesian(atm):
    """geo2cart(0, lon, lat) of every particle: [np][3]"""
    return np.array([geo2cart(0.0, lo, la) for lo, la in zip(atm["lon"].tolist(), atm["lat"].tolist())]).reshape(-1, 3)


def sample_obs(atm, t0, t1, obs_lon, obs_lat, obs_z, dx, dz, qnt_m, kernel=((), ()), xyz=None):
    """the inner loop output.c:640-652 for every observation.  Returns (count, mass, stages): stages[i] = the number of
    particles left after the time window, the latitude band, the distance and the depth test of observation i."""
    kz, kw = [float(v) for v in kernel[0]], [float(v) for v in kernel[1]]
    xyz = cartesian(atm) if xyz is None else xyz
    reach2 = dx * dx
    reach_lat = dx * 180. / (math.pi * RE)
    time, lat, p = atm["time"], atm["lat"], atm["p"]
    in_time = ~((time < t0) | (time > t1))
    count, mass, stages, hits = [], [], [], []
    for lo, la, z in zip(obs_lon, obs_lat, obs_z):
        centre = geo2cart(0.0, float(lo), float(la))
        p_top, p_bottom = P(float(z) + dz), P(float(z) - dz)
        band = in_time & ~(np.abs(float(la) - lat) > reach_lat)
        d0, d1, d2 = centre[0] - xyz[:, 0], centre[1] - xyz[:, 1], centre[2] - xyz[:, 2]
        s = 0.0 + d0 * d0          # dist2: s = 0; s += (a[k] - b[k])^2 for k = 0, 1, 2
        s = s + d1 * d1
        s = s + d2 * d2
        near = band & ~(s > reach2)
        inside = near & ~((p > p_bottom) | (p < p_top)) if dz > 0 else near
        idx = np.nonzero(inside)[0]
        m = 0.0
        if qnt_m >= 0:
            for ip in idx.tolist():   # ascending particle index, one addition after the other
                m += kernel_weight(kz, kw, float(p[ip])) * float(atm["q"][qnt_m][ip])
        count.append(len(idx))
        mass.append(m)
        stages.append((int(in_time.sum()), int(band.sum()), int(near.sum()), len(idx)))
        hits.append(idx)
    return np.array(count, dtype=np.int32), np.array(mass), stages, hits


def station_hits(atm, t, dt_mod, lon, lat, r, stat_t0, stat_t1, qnt_stat, xyz=None):
    """the loop output.c:696-714: (indices listed, rows time / p / lon / lat / q..., flags afterwards, particles skipped
    for their flag although they are in the time windows)"""
    xyz = cartesian(atm) if xyz is None else xyz
    station = geo2cart(0.0, lon, lat)
    t0, t1, reach2 = t - 0.5 * dt_mod, t + 0.5 * dt_mod, r * r
    q = atm["q"].copy()
    listed, rows, skipped = [], [], 0
    for ip in range(len(atm["time"])):
        tp = float(atm["time"][ip])
        if tp < t0 or tp > t1 or tp < stat_t0 or tp > stat_t1:
            continue
        if qnt_stat >= 0 and int(q[qnt_stat][ip]):
            skipped += 1
            continue
        s = 0.0
        for k in range(3):
            s += (station[k] - float(xyz[ip, k])) * (station[k] - float(xyz[ip, k]))
        if s > reach2:
            continue
        if qnt_stat >= 0:
            q[qnt_stat][ip] = 1
        listed.append(ip)
        rows.append([tp, atm["p"][ip], atm["lon"][ip], atm["lat"][ip]] + [q[iq][ip] for iq in range(q.shape[0])])
    return np.array(listed, dtype=np.int32), np.array(rows).reshape(len(listed), 4 + q.shape[0]), q, skipped
