"""Scalar restatement of module_oh_chem (src/mptrac.c:5351-5434) and the SPECIES presets of its constants
(mptrac.c:7291-7383), for the OH chemistry tests.

Two arithmetic modes: "numpy" (the default build's yardstick) and "libm" (the reference-rounding build's: exp, pow
and log10 of the C library through ctypes, IEEE divisions -- Python's own float division is one).  The temperature
and the OH value at the particle come from the oracle's module_meteo (quantities t and oh)."""
import ctypes as C
import math

import numpy as np

AVO = 6.02214e23
RI = 8.3144598

# SPECIES -> (OH_CHEM_REACTION, OH_CHEM[0..3])
PRESETS = {
    "CH4": (2, (2.45e-12, 1775.0, 0.0, 0.0)),
    "CO": (3, (6.9e-33, 2.1, 1.1e-12, -1.3)),
    "NH3": (2, (1.7e-12, 710.0, 0.0, 0.0)),
    "NO": (3, (7.1e-31, 2.6, 3.6e-11, 0.1)),
    "NO2": (3, (1.8e-30, 3.0, 2.8e-11, 0.0)),
    "O3": (2, (1.7e-12, 940.0, 0.0, 0.0)),
    "SO2": (3, (2.9e-31, 4.1, 1.7e-12, -0.2)),
}

_libm = None


def _lib():
    global _libm
    if _libm is None:
        _libm = C.CDLL("libm.so.6")
        for f in ("exp", "log10"):
            getattr(_libm, f).restype = C.c_double
            getattr(_libm, f).argtypes = [C.c_double]
        _libm.pow.restype = C.c_double
        _libm.pow.argtypes = [C.c_double, C.c_double]
    return _libm


def _funcs(mode):
    if mode == "libm":
        L = _lib()
        return L.exp, L.pow, L.log10
    return (lambda x: float(np.exp(x))), (lambda x, y: float(np.power(x, y))), (lambda x: float(np.log10(x)))


def rate(reaction, c, p, t, oh, mode="numpy"):
    """k [OH] M of one particle: pressure p [hPa], temperature t [K], OH volume mixing ratio oh."""
    exp, pw, log10 = _funcs(mode)
    M = AVO * 1e-6 * (p * 100) / (RI * t)
    if reaction == 1:
        k = c[0]
    elif reaction == 2:
        k = c[0] * exp(-c[1] / t)
    elif reaction == 3:
        k0 = c[0] * (pw(298. / t, c[1]) if c[1] > 0 else 1.)
        ki = c[2] * (pw(298. / t, c[3]) if c[3] > 0 else 1.)
        e = log10(k0 * M / ki)
        k = k0 * M / (1. + k0 * M / ki) * pw(0.6, 1. / (1. + e * e))
    else:
        raise ValueError(reaction)
    return k * oh * M


def factor(reaction, c, p, t, oh, dt, mode="numpy"):
    """(aux, rate): the factor exp(-dt rate) the mass and the mixing ratio are multiplied by, and the rate."""
    exp = _funcs(mode)[0]
    r = rate(reaction, c, float(p), float(t), float(oh), mode)
    return exp(-float(dt) * r), r


def apply(q, idx, reaction, c, p, t, oh, dt, mode="numpy"):
    """module_oh_chem on the quantity rows q[nq][np] in place; idx = dict of the qnt_* indices (m, vmr, mloss_oh,
    loss_rate; -1 = absent).  Particles with dt == 0 are left alone."""
    for i in range(q.shape[1]):
        if dt[i] == 0:
            continue
        aux, r = factor(reaction, c, p[i], t[i], oh[i], dt[i], mode)
        if idx.get("m", -1) >= 0:
            m = q[idx["m"], i]
            if idx.get("mloss_oh", -1) >= 0:
                q[idx["mloss_oh"], i] += m * (1 - aux)
            q[idx["m"], i] = m * aux
            if idx.get("loss_rate", -1) >= 0:
                q[idx["loss_rate"], i] += r
        if idx.get("vmr", -1) >= 0:
            q[idx["vmr"], i] *= aux
    return q
