"""Restatement of module_radio_decay, for the radioactive-decay tests.

The step's dt is the one module_timesteps stored (cache->dt).  For every particle with dt != 0 and for each present
activity quantity k (Arn222, Apb210, Abe7, Acs137, Ai131, Axe133; Bq):

    lambda_k = M_LN2 / T_k          (half-life T_k in seconds; one year = 365.25 days)
    e_k      = exp(-lambda_k * dt)
    Be-7, Cs-137, I-131, Xe-133, Rn-222:   A_k <- A_k * e_k
    Pb-210:                                 A_pb <- (A_pb * e_pb) + ((A_rn0 * c_pb) * (e_rn - e_pb))
    with c_pb = lambda_pb / (lambda_pb - lambda_rn)

-- the two-member Bateman solution in activities, the short-lived daughters Po-218 ... Po-214 lumped into the step
Rn-222 -> Pb-210.  A_rn0 is the Rn-222 activity before this step's decay; without Rn-222 the ingrowth term is 0 (and not
evaluated).  The parentheses above are the association the device code uses (mphip_device.hpp: radio_decay): the
reference-rounding build reproduces this restatement's "libm" mode bit for bit.  Nothing else changes: m, vmr, the loss
quantities, absent activities.  A negative dt (DIRECTION -1) takes the same formula.

The constants are kept in one table (HALF_LIFE, mphip_device.hpp: kRadioHalfLife is the same table).  Half-lives from
evaluated nuclear data (ENSDF, as tabulated by the IAEA Live Chart of Nuclides / NNDC NuDat): Rn-222 3.8235 d,
Pb-210 22.20 a, Be-7 53.22 d, Cs-137 30.08 a, I-131 8.0252 d, Xe-133 5.2475 d.  They have not been checked against
the reference's module_radio_decay.

Two arithmetic modes as in tests/refchem.py: "numpy" (numpy's exp) and "libm" (the C library's exp through ctypes)."""
import ctypes as C
import math

import numpy as np

DAY = 86400.0
YEAR = 365.25 * DAY

# quantity names in MPHIP_RN_* slot order, and the half-lives [s]
NAMES = ("Arn222", "Apb210", "Abe7", "Acs137", "Ai131", "Axe133")
HALF_LIFE = (3.8235 * DAY, 22.20 * YEAR, 53.22 * DAY, 30.08 * YEAR, 8.0252 * DAY, 5.2475 * DAY)
RN, PB = 0, 1

LAMBDA = tuple(math.log(2) / T for T in HALF_LIFE)             # (M_LN2 is log(2) rounded: the same double)
C_PB = LAMBDA[PB] / (LAMBDA[PB] - LAMBDA[RN])

_libm = None


def _exp(mode):
    global _libm
    if mode == "libm":
        if _libm is None:
            _libm = C.CDLL("libm.so.6")
            _libm.exp.restype = C.c_double
            _libm.exp.argtypes = [C.c_double]
        f = _libm.exp
        return np.vectorize(lambda x: f(float(x)), otypes=[np.float64])
    return np.exp


def apply(q, idx, dt, mode="numpy"):
    """module_radio_decay on the quantity rows q[nq][np] in place; idx: a sequence of MPHIP_NRADIO row indices in NAMES
    order (-1: absent) or {name: row}.  Particles with dt == 0 are left alone."""
    if isinstance(idx, dict):
        idx = [idx.get(n, -1) for n in NAMES]
    idx = list(idx)
    assert len(idx) == len(NAMES)
    dt = np.asarray(dt, dtype=np.float64)
    live = np.nonzero(dt != 0)[0]
    if len(live) == 0 or all(r < 0 for r in idx):
        return q
    exp = _exp(mode)
    d = dt[live]
    e = {k: exp(-LAMBDA[k] * d) for k, r in enumerate(idx) if r >= 0 or (k == RN and idx[PB] >= 0)}
    rn0 = q[idx[RN], live].copy() if idx[RN] >= 0 else None
    for k, r in enumerate(idx):
        if r < 0:
            continue
        if k == PB:
            a = q[r, live] * e[PB]
            if rn0 is not None:
                a = a + (rn0 * C_PB) * (e[RN] - e[PB])
            q[r, live] = a
        else:
            q[r, live] = q[r, live] * e[k]
    return q


def pb_ingrowth_closed_form(a_rn0, t):
    """Pb-210 activity at time t grown from a pure Rn-222 activity a_rn0 (no Pb-210 at t = 0): the Bateman solution
    A_pb(t) = A_rn0 lambda_pb / (lambda_pb - lambda_rn) (exp(-lambda_rn t) - exp(-lambda_pb t)), written with expm1
    so that it does not share the rounding of apply()'s expression."""
    lr, lp = LAMBDA[RN], LAMBDA[PB]
    return a_rn0 * lp / (lp - lr) * math.exp(-lp * t) * math.expm1(-(lr - lp) * t)
