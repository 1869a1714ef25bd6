"""Scalar restatement of module_tracer_chem and clim_photo, for the tracer chemistry tests.

For every particle with dt != 0: the temperature t, the total ozone column o3c and the O(1D) volume mixing ratio o1d at
the particle (the oracle's module_meteo: quantities t, o3c, o1d), the molecular density M = MOLEC_DENS(p, t), the solar
zenith angle sza = acos(cos_sza(time, lon, lat)) (orc_cos_sza), and for each present quantity of CFC-10, CFC-11, CFC-12
and N2O

    K_o1d = ARRHENIUS(a, b, t) * o1d * M,   K_hv = clim_photo(rate, p, sza, o3c),   q *= exp(-dt (K_hv + K_o1d))

with ARRHENIUS(a, b, t) = a exp(-b / t).  Csf6 has no reaction.  clim_photo clamps p, sza and o3c to the table, finds
the indices with locate_irr (pressure) and locate_reg (sza, o3c) -- the oracle's orc_locate_irr / orc_locate_reg --,
interpolates linearly in pressure at the four (sza, o3c) corners, then in o3c, then in sza, and returns MAX(aux, 0).

Two arithmetic modes as in tests/refchem.py: "numpy" and "libm" (exp and acos of the C library through ctypes)."""
import ctypes as C
import math

import numpy as np

AVO = 6.02214e23
RI = 8.3144598

SPECIES = ("Cccl4", "Cccl3f", "Cccl2f2", "Cn2o")             # MPHIP_TR_CCL4 ... MPHIP_TR_N2O
TABLES = ("ccl4", "ccl3f", "ccl2f2", "n2o")                    # their photolysis tables (clim_photo_t members)
ARRHENIUS = {"Cccl4": (3.30e-10, 0), "Cccl3f": (2.30e-10, 0), "Cccl2f2": (1.40e-10, -25), "Cn2o": (1.19e-10, -20)}

_libm = None
_orc = None
_dp = C.POINTER(C.c_double)


def _lib():
    global _libm
    if _libm is None:
        _libm = C.CDLL("libm.so.6")
        for f in ("exp", "acos"):
            getattr(_libm, f).restype = C.c_double
            getattr(_libm, f).argtypes = [C.c_double]
    return _libm


def _funcs(mode):
    if mode == "libm":
        L = _lib()
        return L.exp, L.acos
    return (lambda x: float(np.exp(x))), math.acos


def oracle():
    global _orc
    if _orc is None:
        from oracle import binding as B
        _orc = B.lib()
    return _orc


def arrhenius(a, b, t, mode="numpy"):
    exp = _funcs(mode)[0]
    return a * exp(-b / t)


class Photo:
    """clim_photo_t: descending p[np] [hPa], ascending sza[nsza] [rad], ascending o3c[no3c] [DU], and
    rates {table name: rate[np][nsza][no3c]}"""

    def __init__(self, p, sza, o3c, rates):
        self.p, self.sza, self.o3c = (np.ascontiguousarray(a, dtype=np.float64) for a in (p, sza, o3c))
        self.rates = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in rates.items()}

    def upload_args(self):
        """the arguments of Simulation.update_clim_photo"""
        return self.p, self.sza, self.o3c, self.rates

    def indices(self, p, sza, o3c):
        """the clamped coordinates and the indices of clim_photo"""
        L = oracle()
        pp, ss, oo = self.p, self.sza, self.o3c
        p_help = pp[-1] if p < pp[-1] else (pp[0] if p > pp[0] else p)
        sza_help = ss[0] if sza < ss[0] else (ss[-1] if sza > ss[-1] else sza)
        o3c_help = oo[0] if o3c < oo[0] else (oo[-1] if o3c > oo[-1] else o3c)
        ip = L.orc_locate_irr(pp.ctypes.data_as(_dp), len(pp), float(p_help))
        isza = L.orc_locate_reg(ss.ctypes.data_as(_dp), len(ss), float(sza_help))
        io3 = L.orc_locate_reg(oo.ctypes.data_as(_dp), len(oo), float(o3c_help))
        return float(p_help), float(sza_help), float(o3c_help), ip, isza, io3

    def rate(self, name, p, sza, o3c):
        """clim_photo(rate, p, sza, o3c) of table `name`"""
        p_help, sza_help, o3c_help, ip, isza, io3 = self.indices(p, sza, o3c)
        r, pp, ss, oo = self.rates[name], self.p, self.sza, self.o3c

        def lin(x0, y0, x1, y1, x):
            return y0 + (y1 - y0) / (x1 - x0) * (x - x0)
        aux00 = lin(pp[ip], r[ip, isza, io3], pp[ip + 1], r[ip + 1, isza, io3], p_help)
        aux01 = lin(pp[ip], r[ip, isza, io3 + 1], pp[ip + 1], r[ip + 1, isza, io3 + 1], p_help)
        aux10 = lin(pp[ip], r[ip, isza + 1, io3], pp[ip + 1], r[ip + 1, isza + 1, io3], p_help)
        aux11 = lin(pp[ip], r[ip, isza + 1, io3 + 1], pp[ip + 1], r[ip + 1, isza + 1, io3 + 1], p_help)
        aux0 = lin(oo[io3], aux00, oo[io3 + 1], aux01, o3c_help)
        aux1 = lin(oo[io3], aux10, oo[io3 + 1], aux11, o3c_help)
        aux = lin(ss[isza], aux0, ss[isza + 1], aux1, sza_help)
        return max(float(aux), 0.0)


def synthetic_photo(seed, np_=16, nsza=13, no3c=9, negative=True):
    """A table shaped like the reference's: pressures 500 ... 0.5 hPa, sza 0.2 ... 1.64 rad, o3c 260 ... 340 DU; rates
    that grow with height and sunlight, some entries negative where `negative` (clim_photo's MAX(aux, 0))"""
    rng = np.random.default_rng(seed)
    p = 500.0 * np.exp(-np.arange(np_) * (np.log(1000.0) / (np_ - 1)))
    sza = 0.2 + 0.12 * np.arange(nsza)
    o3c = 260.0 + 10.0 * np.arange(no3c)
    rates = {}
    for k, name in enumerate(TABLES):
        base = (10.0 ** (-9.0 + 3.5 * np.arange(np_) / (np_ - 1)))[:, None, None]
        light = np.cos(np.minimum(sza, 1.55))[None, :, None] * (1.2 - (o3c - 260.0) / 400.0)[None, None, :]
        noise = rng.uniform(-0.3 if negative else 0.5, 1.0, (np_, nsza, no3c))
        rates[name] = (k + 1) * base * light * noise
    return Photo(p, sza, o3c, rates)


def sza_at(time, lon, lat, mode="numpy"):
    acos = _funcs(mode)[1]
    return acos(oracle().orc_cos_sza(float(time), float(lon), float(lat)))


def apply(q, idx, photo, time, p, lon, lat, t, o1d, o3c, dt, mode="numpy"):
    """module_tracer_chem on the quantity rows q[nq][np] in place; idx: {species name: row} (-1 / missing = absent).
    t, o1d, o3c: at each particle.  Particles with dt == 0 are left alone."""
    exp = _funcs(mode)[0]
    present = [(name, TABLES[k], idx[name]) for k, name in enumerate(SPECIES) if idx.get(name, -1) >= 0]
    if not present:
        return q
    for i in range(q.shape[1]):
        if dt[i] == 0:
            continue
        ti = float(t[i])
        M = AVO * 1e-6 * (float(p[i]) * 100) / (RI * ti)
        sza = sza_at(time[i], lon[i], lat[i], mode)
        for name, table, row in present:
            a, b = ARRHENIUS[name]
            k_o1d = arrhenius(a, b, ti, mode) * float(o1d[i]) * M
            k_hv = photo.rate(table, float(p[i]), sza, float(o3c[i]))
            q[row, i] *= exp(-float(dt[i]) * (k_hv + k_o1d))
    return q
