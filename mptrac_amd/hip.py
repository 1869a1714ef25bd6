"""ctypes binding of the C ABI in include/mptrac_hip.h and a thin host-side
mirror of the reference's high-level interface (``mptrac_alloc`` ...
``mptrac_update_host``, src/mptrac.h:7246-7736) on top of it.

There is no CPU fallback: if the HIP library or a device is missing, creating
a ``Simulation`` raises.
"""
import atexit
import ctypes as C
import os
import sys
import weakref

import numpy as np

from . import build as _build
from .ctl import (HIP_CTL_FIELDS, RADIO_ACTIVITIES, TRACER_SERIES, ZONAL_MEANS, fill_ctl, make_ctl_struct,
                  radio_from_quantities)
from .synth import FIELDS_2D, FIELDS_3D, FIELDS_ML

NQ_MAX = 16
INTPOL_2D = 256     # MPHIP_INTPOL_2D: the field index of mphip_intpol_met names a surface field
MOD = {
    "timesteps": 1 << 0, "position": 1 << 1, "advect": 1 << 2, "diff_turb": 1 << 3, "diff_meso": 1 << 4,
    "convection": 1 << 5, "sedi": 1 << 6, "position2": 1 << 7, "loss_zero": 1 << 8, "decay": 1 << 9,
    "wet_depo": 1 << 10, "dry_depo": 1 << 11, "advect_init": 1 << 12, "diff_pbl": 1 << 13, "meteo": 1 << 14,
    "isosurf": 1 << 15, "sort": 1 << 16, "mixing": 1 << 17, "bound_cond": 1 << 18, "bound_cond2": 1 << 19,
    "isosurf_init": 1 << 20, "oh_chem": 1 << 21, "chem_grid": 1 << 22, "h2o2_chem": 1 << 23,
    "tracer_chem": 1 << 24, "radio_decay": 1 << 25, "radio_depo": 1 << 26,
}

MphipCtl = make_ctl_struct("MphipCtl", HIP_CTL_FIELDS)
_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)


class MphipMet(C.Structure):
    _fields_ = [("time", C.c_double), ("coord_type", C.c_int), ("nx", C.c_int), ("ny", C.c_int),
                ("np", C.c_int), ("npl", C.c_int), ("lon", _dp), ("lat", _dp), ("p", _dp),
                ("sx", C.c_longlong), ("sy", C.c_longlong), ("sx2", C.c_longlong),
                ("sx_ml", C.c_longlong), ("sy_ml", C.c_longlong),
                ("f3", _fp * len(FIELDS_3D)), ("f2", _fp * len(FIELDS_2D))]


class MphipPrep(C.Structure):
    """mphip_prep_t: the options of mphip_derive_met."""
    _fields_ = [("met_pbl", C.c_int), ("met_pbl_min", C.c_double), ("met_pbl_max", C.c_double),
                ("met_geopot_sx", C.c_int), ("met_geopot_sy", C.c_int), ("met_cloud_min", C.c_double),
                ("met_tropo", C.c_int), ("met_tropo_pv", C.c_double), ("met_tropo_theta", C.c_double),
                ("met_tropo_spline", C.c_int)]


class MphipMetOut(C.Structure):
    """mphip_met_out_t: the output arrays of mphip_derive_met (strides of the input view)."""
    _fields_ = [("f3", _fp * len(FIELDS_3D)), ("f2", _fp * len(FIELDS_2D))]


PREP = {"geopot": 1, "o3c": 2, "pbl": 4, "cloud": 8, "cape": 16, "pv": 32, "tropo": 64}
PREP_OUTPUTS = {"geopot": ("z",), "o3c": ("o3c",), "pbl": ("pbl",), "cloud": ("pct", "pcb", "cl"),
                "cape": ("plcl", "plfc", "pel", "cape", "cin"), "pv": ("pv",), "tropo": ("pt", "tt", "zt", "h2ot")}


class MphipRegrid(C.Structure):
    """mphip_regrid_t: the options of mphip_regrid_met."""
    _fields_ = [("met_np", C.c_int), ("met_p", _dp), ("met_dx", C.c_int), ("met_dy", C.c_int), ("met_dp", C.c_int),
                ("met_sx", C.c_int), ("met_sy", C.c_int), ("met_sp", C.c_int)]


class MphipRegridOut(C.Structure):
    """mphip_regrid_out_t: the output arrays of mphip_regrid_met, their strides and the output axes."""
    _fields_ = [("sx", C.c_longlong), ("sy", C.c_longlong), ("sx2", C.c_longlong), ("lon", _dp), ("lat", _dp), ("p", _dp),
                ("f3", _fp * len(FIELDS_3D)), ("f2", _fp * len(FIELDS_2D))]


REGRID = {"ml2pl": 1, "sample": 2}
REGRID_ML = ("t", "u", "v", "w", "h2o", "o3", "lwc", "rwc", "iwc", "swc", "cc")      # what ML2PL regrids
REGRID_PL = REGRID_ML + ("z", "pv")                                                  # what SAMPLE takes


class MphipDetrend(C.Structure):
    """mphip_detrend_t: the option of mphip_detrend_met."""
    _fields_ = [("met_detrend", C.c_double)]


DETREND_FIELDS = ("t", "u", "v", "w")

INGEST = {"decode": 1, "extrapolate": 2, "polar": 4, "periodic": 8}
INGEST_ALL = 15
RAW_FLOAT, RAW_SHORT = 1, 2       # MPHIP_RAW_FLOAT, MPHIP_RAW_SHORT


class MphipRaw(C.Structure):
    """mphip_raw_t: one field as a netCDF file stores it."""
    _fields_ = [("data", C.c_void_p), ("type", C.c_int), ("lnsp", C.c_int), ("scale_factor", C.c_float),
                ("add_offset", C.c_float), ("fill_f", C.c_float), ("miss_f", C.c_float), ("fill_s", C.c_short),
                ("miss_s", C.c_short), ("scl", C.c_float)]


class MphipIngestRaw(C.Structure):
    """mphip_ingest_raw_t: the raw descriptors of mphip_ingest_met, one per field slot."""
    _fields_ = [("f3", MphipRaw * len(FIELDS_3D)), ("f2", MphipRaw * len(FIELDS_2D))]


_up = C.POINTER(C.c_ushort)


class MphipMetPacked(C.Structure):
    """mphip_met_packed_t: a snapshot some of whose level fields are 16-bit codes (MET_TYPE 2)."""
    _fields_ = [("base", MphipMet), ("q3", _up * len(FIELDS_3D)), ("scl", _dp * len(FIELDS_3D)), ("off", _dp * len(FIELDS_3D)),
                ("lo", C.c_float * len(FIELDS_3D)), ("hi", C.c_float * len(FIELDS_3D))]


# the limits the reader of the binary files applies to a level field (every other field: PACK_LIMITS_OPEN)
PACK_LIMITS_OPEN = (-1e34, 1e34)
PACK_LIMITS = {"t": (0., 1e34), "h2o": (0., 1e34), "o3": (0., 1e34), "lwc": (0., 1e34), "rwc": (0., 1e34), "iwc": (0., 1e34),
               "swc": (0., 1e34), "cc": (0., 1.)}


class Snapshot:
    """What Simulation.regrid_met returns: the axes (float64) and the float32 fields of the new shape, named as in
    synth.Met (`strides` = (sx, sy, sx2) in floats where the arrays are views into larger ones)."""

    def __init__(self, time, coord_type, lon, lat, p, f3, f2, strides=None):
        self.time, self.coord_type = float(time), int(coord_type)
        self.lon, self.lat, self.p = lon, lat, p
        self.nx, self.ny, self.np = len(lon), len(lat), len(p)
        self.npl = self.np
        self.f3, self.f2 = f3, f2
        if strides is not None:
            self.strides = strides


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)

_lib = None


class MphipBox(C.Structure):
    """mphip_box_t: a regular lon / lat / log-pressure-height box grid (CSI, profiles)."""
    _fields_ = [("lon0", C.c_double), ("lon1", C.c_double), ("nx", C.c_int), ("lat0", C.c_double), ("lat1", C.c_double),
                ("ny", C.c_int), ("z0", C.c_double), ("z1", C.c_double), ("nz", C.c_int)]


class MphipSelect(C.Structure):
    """mphip_select_t: which particles mphip_select_atm returns (index range and stride, ANDed range and distance tests)."""
    _fields_ = [("first", C.c_longlong), ("last", C.c_longlong), ("stride", C.c_longlong),
                ("use_time", C.c_int), ("use_z", C.c_int), ("use_lon", C.c_int), ("use_lat", C.c_int), ("use_near", C.c_int),
                ("t0", C.c_double), ("t1", C.c_double), ("z0", C.c_double), ("z1", C.c_double),
                ("lon0", C.c_double), ("lon1", C.c_double), ("lat0", C.c_double), ("lat1", C.c_double),
                ("near_lon", C.c_double), ("near_lat", C.c_double), ("near_r", C.c_double)]


class MphipError(RuntimeError):
    pass


_LIVE = weakref.WeakSet()     # contexts not closed yet: closed at exit while the HIP runtime is still up


@atexit.register
def _close_live_contexts():
    for sim in list(_LIVE):
        try:
            sim.close()
        except Exception:
            pass


def lib_path():
    """The library load() takes: MPHIP_LIB, or with MPTRAC_AMD_EXACT=1 the reference-rounding build, else the default."""
    if os.environ.get("MPHIP_LIB"):
        return os.environ["MPHIP_LIB"]
    return _build.EXACT_LIB if _build.exact_requested() else _build.HIP_LIB


def load(build=True):
    """Load libmptrac_hip.so (building it first if sources are newer)."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.build_hip() if build else lib_path()
    if not os.path.exists(path):
        raise MphipError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(path)
    L.mphip_sizeof_ctl.restype = C.c_size_t
    L.mphip_sizeof_met.restype = C.c_size_t
    L.mphip_version.restype = C.c_char_p
    L.mphip_last_error.restype = C.c_char_p
    L.mphip_last_error.argtypes = [C.c_void_p]
    L.mphip_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    L.mphip_destroy.argtypes = [C.c_void_p]
    L.mphip_destroy.restype = None
    L.mphip_update_ctl.argtypes = [C.c_void_p, C.POINTER(MphipCtl)]
    L.mphip_update_clim.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, C.c_int]
    L.mphip_update_clim_zm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp]
    L.mphip_update_clim_ts.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp]
    L.mphip_update_clim_photo.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, C.POINTER(_dp)]
    L.mphip_update_met.argtypes = [C.c_void_p, C.c_int, C.POINTER(MphipMet)]
    L.mphip_swap_met.argtypes = [C.c_void_p]
    L.mphip_prefetch_met.argtypes = [C.c_void_p, C.POINTER(MphipMet)]
    L.mphip_commit_met.argtypes = [C.c_void_p]
    L.mphip_prefetch_done.argtypes = [C.c_void_p]
    L.mphip_discard_prefetch.argtypes = [C.c_void_p]
    if hasattr(L, "mphip_derive_met"):      # (absent from libraries built before the meteo preprocessing: A/B runs through MPHIP_LIB)
        L.mphip_derive_met.argtypes = [C.c_void_p, C.POINTER(MphipMet), C.c_uint, C.POINTER(MphipPrep), C.POINTER(MphipMetOut)]
    if hasattr(L, "mphip_regrid_met"):      # (absent from libraries built before the regridding: A/B runs through MPHIP_LIB)
        L.mphip_regrid_met.argtypes = [C.c_void_p, C.POINTER(MphipMet), C.c_uint, C.POINTER(MphipRegrid), C.POINTER(MphipRegridOut)]
        L.mphip_regrid_shape.argtypes = [C.POINTER(MphipMet), C.c_uint, C.POINTER(MphipRegrid), C.POINTER(C.c_int),
                                         C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mphip_sizeof_regrid.restype = C.c_size_t
        if L.mphip_sizeof_regrid() != C.sizeof(MphipRegrid):
            raise MphipError("mphip_regrid_t layout mismatch between header and Python mirror")
    if hasattr(L, "mphip_detrend_met"):     # (absent from libraries built before the detrending: A/B runs through MPHIP_LIB)
        L.mphip_detrend_met.argtypes = [C.c_void_p, C.POINTER(MphipMet), C.POINTER(MphipDetrend), C.POINTER(MphipRegridOut)]
        L.mphip_sizeof_detrend.restype = C.c_size_t
        if L.mphip_sizeof_detrend() != C.sizeof(MphipDetrend):
            raise MphipError("mphip_detrend_t layout mismatch between header and Python mirror")
    if hasattr(L, "mphip_ingest_met"):      # (absent from libraries built before the ingest: A/B runs through MPHIP_LIB)
        L.mphip_ingest_met.argtypes = [C.c_void_p, C.POINTER(MphipMet), C.POINTER(MphipIngestRaw), C.c_uint,
                                       C.POINTER(MphipRegridOut)]
        L.mphip_ingest_shape.argtypes = [C.POINTER(MphipMet), C.c_uint, C.POINTER(C.c_int)]
        L.mphip_sizeof_ingest_raw.restype = C.c_size_t
        if L.mphip_sizeof_ingest_raw() != C.sizeof(MphipIngestRaw):
            raise MphipError("mphip_ingest_raw_t layout mismatch between header and Python mirror")
    if hasattr(L, "mphip_update_met_packed"):      # (absent from libraries built before the packed files: A/B runs through MPHIP_LIB)
        L.mphip_update_met_packed.argtypes = [C.c_void_p, C.c_int, C.POINTER(MphipMetPacked)]
        L.mphip_prefetch_met_packed.argtypes = [C.c_void_p, C.POINTER(MphipMetPacked)]
        L.mphip_unpack_met.argtypes = [C.c_void_p, C.POINTER(MphipMetPacked), C.POINTER(MphipMet)]
        L.mphip_pack_met.argtypes = [C.c_void_p, C.POINTER(MphipMet), C.POINTER(MphipMetPacked)]
        L.mphip_sizeof_met_packed.restype = C.c_size_t
        if L.mphip_sizeof_met_packed() != C.sizeof(MphipMetPacked):
            raise MphipError("mphip_met_packed_t layout mismatch between header and Python mirror")
    if hasattr(L, "mphip_intpol_met"):      # (absent from libraries built before the point interpolation: A/B runs through MPHIP_LIB)
        L.mphip_intpol_met.argtypes = [C.c_void_p, C.c_longlong, _dp, C.c_longlong, _dp, _dp, _dp, C.c_int, C.POINTER(C.c_int), _dp]
    if hasattr(L, "mphip_sizeof_prep"):     # (absent from libraries built before pv and the tropopause: they read the old members)
        L.mphip_sizeof_prep.restype = C.c_size_t
        if L.mphip_sizeof_prep() != C.sizeof(MphipPrep):
            raise MphipError("mphip_prep_t layout mismatch between header and Python mirror")
    L.mphip_update_atm.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_longlong, C.c_int,
                                   _dp, _dp, _dp, _dp, C.POINTER(_dp)]
    L.mphip_get_atm.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, C.POINTER(_dp)]
    L.mphip_update_quantity.argtypes = [C.c_void_p, C.c_int, _dp]
    L.mphip_update_cache.argtypes = [C.c_void_p, _fp, C.POINTER(C.c_uint64)]
    L.mphip_get_cache.argtypes = [C.c_void_p, _fp, _dp, C.POINTER(C.c_uint64)]
    L.mphip_update_iso.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int]
    L.mphip_get_iso.argtypes = [C.c_void_p, _dp]
    L.mphip_run_timestep.argtypes = [C.c_void_p, C.c_double]
    L.mphip_run_timesteps.argtypes = [C.c_void_p, C.c_double, C.c_int]
    L.mphip_module.argtypes = [C.c_void_p, C.c_uint, C.c_double]
    L.mphip_get_sort.argtypes = [C.c_void_p, _dp, C.POINTER(C.c_int)]
    if hasattr(L, "mphip_get_sort_counts"):      # (absent from libraries built before the sort counters: Simulation._sort_counts says so)
        L.mphip_get_sort_counts.argtypes = [C.c_void_p] + [C.POINTER(C.c_longlong)] * 3
    L.mphip_grid_sums.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_int), _dp, _dp]
    L.mphip_set_grid_kernel.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    _ip = C.POINTER(C.c_int)
    L.mphip_box_sums.argtypes = [C.c_void_p, C.POINTER(MphipBox), C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp]
    L.mphip_sample_obs.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double,
                                   C.c_int, _dp, _dp, _ip, _dp]
    L.mphip_station_hits.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                     C.c_int, C.c_int, _ip, _ip, _dp]
    if hasattr(L, "mphip_select_atm"):      # (absent from libraries built before the selection: A/B runs through MPHIP_LIB)
        L.mphip_select_atm.argtypes = [C.c_void_p, C.POINTER(MphipSelect), C.c_longlong, C.POINTER(C.c_longlong), _ip,
                                       _dp, _dp, _dp, _dp, C.POINTER(_dp)]
    L.mphip_set_radio_decay.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    if hasattr(L, "mphip_set_radio_depo"):      # (absent from libraries built before module_radio_depo: A/B runs through MPHIP_LIB)
        L.mphip_set_radio_depo.argtypes = [C.c_void_p, C.c_int, C.POINTER(MphipBox)]
        L.mphip_get_radio_depo.argtypes = [C.c_void_p, _dp, _dp, _dp]
        L.mphip_get_shortcuts.argtypes = [C.c_void_p, _dp]
    L.mphip_set_allreduce.argtypes = [C.c_void_p, ALLREDUCE_FN, C.c_void_p]
    L.mphip_comm_unique_id.argtypes = [C.c_void_p]
    L.mphip_comm_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.mphip_comm_destroy.argtypes = [C.c_void_p]
    L.mphip_comm_query.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mphip_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
    L.mphip_synchronize.argtypes = [C.c_void_p]
    L.mphip_profile_begin.argtypes = [C.c_void_p]
    L.mphip_profile_end.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), _dp]
    L.mphip_test_sincosf.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, _fp, _fp]
    L.mphip_test_rng.argtypes = [C.c_void_p, C.c_uint64, C.c_longlong, C.c_int, _dp]
    L.mphip_test_piece.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp]
    if hasattr(L, "mphip_test_libm"):      # (absent from libraries built before round 6: A/B runs through MPHIP_LIB)
        L.mphip_test_libm.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_longlong, _dp]
    if hasattr(L, "mphip_test_meso_table"):      # (absent from libraries built before round 8)
        L.mphip_test_meso_table.argtypes = [C.c_void_p, _fp, C.c_size_t]
    if L.mphip_sizeof_ctl() != C.sizeof(MphipCtl):
        raise MphipError("mphip_ctl_t layout mismatch between header and Python mirror")
    if L.mphip_sizeof_met() != C.sizeof(MphipMet):
        raise MphipError("mphip_met_t layout mismatch between header and Python mirror")
    _lib = L
    return L


def _ptr(a, t):
    return a.ctypes.data_as(t)


def _bits(table, what):
    """`what` of a meteo call: a name of `table`, several of them, or the OR of their bits itself."""
    if isinstance(what, str):
        what = (what,)
    return what if isinstance(what, int) else sum(table[w] for w in set(what))


def _name_out(mo, f, a, shape=None, strides=None, check=True):
    """Name the array `a` as field f of the out-structure `mo` (f3 or f2 by the field's kind).  Checked first, unless the
    call is made for its refusal alone: float32 and, where given, the shape and the strides in bytes."""
    if check:
        assert a.dtype == np.float32 and shape in (None, a.shape) and strides in (None, a.strides), f
    if f in FIELDS_3D:
        mo.f3[FIELDS_3D.index(f)] = _ptr(a, _fp)
    else:
        mo.f2[FIELDS_2D.index(f)] = _ptr(a, _fp)


def shard_range(n, rank, world):
    """Contiguous index range [lo, hi) of rank `rank`."""
    return (n * rank) // world, (n * (rank + 1)) // world


def timestep_range(direction, dt_mod, t_stop, tmin, tmax):
    """(t_start, t_stop) of module_timesteps_init (src/mptrac.c:6046-6073) from the smallest / largest particle time:
    the run starts at the first release in the direction of travel, rounded outwards to the DT_MOD raster (floor for a
    forward, ceil for a backward run), and ends at the last one unless T_STOP was given (<= 1e99)."""
    if direction == 1:
        t_start = tmin
        if t_stop > 1e99:
            t_stop = tmax
    else:
        t_start = tmax
        if t_stop > 1e99:
            t_stop = tmin
    if direction * (t_stop - t_start) <= 0:
        raise MphipError("Nothing to do! Check T_STOP and DIRECTION!")
    t_start = float((np.floor if direction == 1 else np.ceil)(t_start / dt_mod) * dt_mod)
    return t_start, float(t_stop)


class Simulation:
    """Host-side handle: one device context + the reference's call sequence.

    ``atm`` is a dict with float64 arrays time, p, lon, lat and q[nq][np]
    holding *all* particles; this process uploads its shard
    ``[lo, hi)`` (default: everything).
    """

    def __init__(self, ctl_kw, clim, met0, met1, atm, device=0, shard=None, rng_ctr=0, n_total=None):
        self.L = load()
        self.h = C.c_void_p()
        rc = self.L.mphip_create(C.byref(self.h), device)
        if rc:
            raise MphipError(f"mphip_create failed with code {rc} (no usable HIP device?)")
        self.ctl = fill_ctl(MphipCtl(), **ctl_kw)
        self._cb = None
        _LIVE.add(self)
        self._mets = [None, None]
        self._next_met = None
        time, lat, tropo = clim[:3]
        tropo = np.ascontiguousarray(tropo, dtype=np.float64)
        self._chk(self.L.mphip_update_clim(self.h, len(time), len(lat),
                                           _ptr(np.ascontiguousarray(time, dtype=np.float64), _dp),
                                           _ptr(np.ascontiguousarray(lat, dtype=np.float64), _dp),
                                           _ptr(tropo, _dp), tropo.shape[1]))
        # zonal-mean climatologies: optional fourth element {name: (time, p, lat, vmr[ntime][np][nlat])}
        # ... and trace-gas time series {name: (time, vmr)}, and the photolysis rates {"photo": (p, sza, o3c, rates)}
        for name, tab in (clim[3] if len(clim) > 3 else {}).items():
            if name == "photo":
                self.update_clim_photo(*tab)
            elif name in TRACER_SERIES:
                self.update_clim_ts(name, *tab)
            else:
                self.update_clim_zm(name, *tab)
        self.update_ctl()
        self.set_met(0, met0)
        self.set_met(1, met1)
        # n_total given: `atm` holds only this process's range [lo, hi) of a
        # simulation with n_total particles; otherwise `atm` holds all of them
        self.atm_is_local = n_total is not None
        self.n_total = n_total if self.atm_is_local else len(atm["time"])
        self.lo, self.hi = shard if shard is not None else (0, self.n_total)
        self.n = self.hi - self.lo
        self.nq = self.ctl.nq
        self.update_atm(atm)
        ctr = C.c_uint64(rng_ctr)
        self._chk(self.L.mphip_update_cache(self.h, None, C.byref(ctr)))

    def update_clim_zm(self, name, time=(), p=(), lat=(), vmr=()):
        """A zonal-mean climatology of clim_t for module_meteo (hno3, oh, h2o2, ho2, o1d); no nodes: removed."""
        time, p, lat, vmr = (np.ascontiguousarray(a, dtype=np.float64) for a in (time, p, lat, vmr))
        if len(time):
            assert vmr.shape == (len(time), len(p), len(lat))
        self._chk(self.L.mphip_update_clim_zm(self.h, ZONAL_MEANS.index(name), len(time), len(p), len(lat),
                                              _ptr(time, _dp), _ptr(p, _dp), _ptr(lat, _dp), _ptr(vmr, _dp)))

    def update_clim_ts(self, name, time=(), vmr=()):
        """Surface time series of a trace gas for module_bound_cond (ccl4, ccl3f, ccl2f2, n2o, sf6); no nodes: removed."""
        time, vmr = (np.ascontiguousarray(a, dtype=np.float64) for a in (time, vmr))
        assert time.shape == vmr.shape
        self._chk(self.L.mphip_update_clim_ts(self.h, TRACER_SERIES.index(name), len(time), _ptr(time, _dp), _ptr(vmr, _dp)))

    def update_clim_photo(self, p=(), sza=(), o3c=(), rates=None):
        """Photolysis rates of clim_t for module_tracer_chem: descending pressures [hPa], ascending solar zenith
        angles [rad] and total ozone columns [DU], and {name: rate[np][nsza][no3c]} for some of ccl4, ccl3f, ccl2f2,
        n2o (TRACER_SERIES names; sf6 has none).  No pressures: removed."""
        p, sza, o3c = (np.ascontiguousarray(a, dtype=np.float64) for a in (p, sza, o3c))
        rates = dict(rates or {})
        keep = []
        ptrs = (_dp * len(TRACER_SERIES))()
        for name, tab in rates.items():
            tab = np.ascontiguousarray(tab, dtype=np.float64)
            assert tab.shape == (len(p), len(sza), len(o3c)), name
            keep.append(tab)
            ptrs[TRACER_SERIES.index(name)] = _ptr(tab, _dp)
        self._chk(self.L.mphip_update_clim_photo(self.h, len(p), len(sza), len(o3c), _ptr(p, _dp), _ptr(sza, _dp),
                                                 _ptr(o3c, _dp), ptrs))

    # -- plumbing -----------------------------------------------------------
    def _chk(self, rc):
        if rc:
            raise MphipError(self.L.mphip_last_error(self.h).decode())

    def close(self):
        _LIVE.discard(self)
        if self.h:
            self.L.mphip_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        # not at interpreter shutdown: the HIP runtime may already be gone then (the atexit hook below
        # has closed every live context before that)
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    # -- mptrac_update_device ------------------------------------------------
    def update_ctl(self):
        self._chk(self.L.mphip_update_ctl(self.h, C.byref(self.ctl)))

    def _met_struct(self, met):
        m = MphipMet()
        m.time, m.coord_type, m.nx, m.ny, m.np = met.time, met.coord_type, met.nx, met.ny, met.np
        m.lon, m.lat, m.p = _ptr(met.lon, _dp), _ptr(met.lat, _dp), _ptr(met.p, _dp)
        # (`strides` = (sx, sy, sx2) in floats: a view into arrays of the reference's fixed extents; derive_met)
        m.sx, m.sy, m.sx2 = getattr(met, "strides", None) or (met.ny * met.np, met.np, met.ny)
        m.npl = met.npl if any(k in met.f3 for k in FIELDS_ML) else 0
        m.sx_ml, m.sy_ml = getattr(met, "strides_ml", None) or (met.ny * met.npl, met.npl)
        for i, k in enumerate(FIELDS_3D):
            m.f3[i] = _ptr(met.f3[k], _fp) if k in met.f3 else None
        for i, k in enumerate(FIELDS_2D):
            m.f2[i] = _ptr(met.f2[k], _fp) if k in met.f2 else None
        return m

    def _shape_refused(self, which, mo, out, out_strides, call):
        """mphip_<which>_shape refused the grid or `what`: `call`, the mphip_<which>_met of the same arguments, is made for
        its message, with the caller's arrays all the same (a refused call writes nothing)."""
        mo.sx, mo.sy, mo.sx2 = out_strides or (0, 0, 0)
        for f, a in (out or {}).items():
            if a is not None:
                _name_out(mo, f, a, check=False)
        self._chk(call())
        raise MphipError(f"mphip_{which}_shape refused what mphip_{which}_met accepts")

    def derive_met(self, met, what, out=None, **opts):
        """The derived fields of the meteo preprocessing (mphip_derive_met).  `met`: a snapshot as synthetic_met returns
        it, or a strided view -- any object with its attributes whose f3 / f2 arrays are NumPy views [nx][ny][np] /
        [nx][ny] into larger float32 arrays (last axis contiguous) and which names their strides in floats as
        `strides` = (sx, sy, sx2).  `what`: names among geopot, o3c, pbl, cloud, cape, pv, tropo (or the OR of their
        MPHIP_PREP_* bits).  Options: met_pbl (3), met_pbl_min (0.1), met_pbl_max (5.0), met_geopot_sx, met_geopot_sy (-1:
        automatic), met_cloud_min (0), met_tropo (3), met_tropo_pv (3.5), met_tropo_theta (380), met_tropo_spline (1).
        `out`: {name: float32 array with the strides of the input} to write into (tests); by default new arrays.  Returns
        {name: array} of the fields of the requested bits."""
        bits = _bits(PREP, what)
        o = MphipPrep(int(opts.pop("met_pbl", 3)), float(opts.pop("met_pbl_min", 0.1)), float(opts.pop("met_pbl_max", 5.0)),
                      int(opts.pop("met_geopot_sx", -1)), int(opts.pop("met_geopot_sy", -1)), float(opts.pop("met_cloud_min", 0.0)),
                      int(opts.pop("met_tropo", 3)), float(opts.pop("met_tropo_pv", 3.5)), float(opts.pop("met_tropo_theta", 380.)),
                      int(opts.pop("met_tropo_spline", 1)))
        if opts:
            raise TypeError(f"unknown options {sorted(opts)}")
        m = self._met_struct(met)
        like3 = next(iter(met.f3.values()), None)
        like2 = next(iter(met.f2.values()), None)
        res = {}
        mo = MphipMetOut()
        for name, fields in PREP_OUTPUTS.items():
            for f in fields:
                three = f in FIELDS_3D
                like = like3 if three else like2
                if out is not None and f in out:        # (passed whether requested or not: the library must leave it alone)
                    a = out[f]
                elif not bits & PREP[name] or like is None:
                    continue
                elif like.flags["C_CONTIGUOUS"]:
                    a = np.empty_like(like)
                elif three:      # a strided view: allocate the enclosing extents, hand out the same view
                    a = np.empty((met.nx, m.sx // m.sy, m.sy), dtype=np.float32)[:, :met.ny, :met.np]
                else:
                    a = np.empty((met.nx, m.sx2), dtype=np.float32)[:, :met.ny]
                _name_out(mo, f, a, strides=like.strides)
                if bits & PREP[name]:
                    res[f] = a
        self._chk(self.L.mphip_derive_met(self.h, C.byref(m), bits, C.byref(o), C.byref(mo)))
        return res

    def regrid_met(self, met, what, out=None, out_strides=None, **opts):
        """Model levels to pressure levels and / or smoothing with down-sampling (mphip_regrid_met).  `met`: a snapshot
        with the conventions of derive_met; for ml2pl its level fields have npl levels, f3["pl"] is the pressure (a view
        names its strides as `strides_ml` = (sx_ml, sy_ml)) and `p` is not read.  `what`: names among ml2pl, sample (or
        the OR of their MPHIP_REGRID_* bits).  Options: met_p (the target levels of ml2pl), met_dx, met_dy, met_dp, met_sx,
        met_sy, met_sp (1).  `out`: {name: float32 array of the new shape to write into, or None to leave a field out}
        -- views into larger arrays name their strides in floats as `out_strides` = (sx, sy, sx2), which then hold for
        every output array (tests; in-place use); by default new compact arrays.  Returns a Snapshot of the new shape."""
        bits = _bits(REGRID, what)
        met_p = np.ascontiguousarray(opts.pop("met_p", ()), dtype=np.float64)
        o = MphipRegrid(len(met_p), _ptr(met_p, _dp) if len(met_p) else None,
                        *(int(opts.pop(k, 1)) for k in ("met_dx", "met_dy", "met_dp", "met_sx", "met_sy", "met_sp")))
        if opts:
            raise TypeError(f"unknown options {sorted(opts)}")
        m = self._met_struct(met)
        if bits & REGRID["ml2pl"]:
            m.npl = met.npl         # (also without pl: that refusal is the library's)
        mo = MphipRegridOut()
        n = [C.c_int(0) for _ in range(3)]
        if self.L.mphip_regrid_shape(C.byref(m), bits, C.byref(o), *(C.byref(k) for k in n)):
            self._shape_refused("regrid", mo, out, out_strides,
                                lambda: self.L.mphip_regrid_met(self.h, C.byref(m), bits, C.byref(o), C.byref(mo)))
        nx2, ny2, np2 = (k.value for k in n)
        mo.sx, mo.sy, mo.sx2 = out_strides or (ny2 * np2, np2, ny2)
        lon, lat, p = (np.empty(k, dtype=np.float64) for k in (nx2, ny2, np2))
        mo.lon, mo.lat, mo.p = _ptr(lon, _dp), _ptr(lat, _dp), _ptr(p, _dp)
        out = dict(out or {})
        f3, f2 = {}, {}
        for f in (REGRID_ML if bits & REGRID["ml2pl"] else REGRID_PL):
            if f in out or f in met.f3:
                a = out[f] if f in out else np.empty((nx2, ny2, np2), dtype=np.float32)
                if a is None:
                    continue
                _name_out(mo, f, a, (nx2, ny2, np2), (4 * mo.sx, 4 * mo.sy, 4))
                if f in met.f3:
                    f3[f] = a
        for f in FIELDS_2D:
            if f in out or f in met.f2:
                a = out[f] if f in out else np.empty((nx2, ny2), dtype=np.float32)
                if a is None:
                    continue
                _name_out(mo, f, a, (nx2, ny2), (4 * mo.sx2, 4))
                if f in met.f2:
                    f2[f] = a
        self._chk(self.L.mphip_regrid_met(self.h, C.byref(m), bits, C.byref(o), C.byref(mo)))
        return Snapshot(met.time, met.coord_type, lon, lat, p, f3, f2, out_strides)

    def detrend_met(self, met, met_detrend, fields=None, out=None, out_strides=None):
        """Detrending (mphip_detrend_met): the Gaussian-weighted horizontal mean of full width at half maximum
        `met_detrend` [km] is subtracted from t, u, v and w.  `met`: a pressure-level snapshot with the conventions of
        derive_met.  `fields`: the names to detrend (default: those of t, u, v, w the snapshot has).  `out`: {name:
        float32 array of the snapshot's shape to write into} -- an input array itself for in-place use; views into
        larger arrays name their strides in floats as `out_strides` = (sx, sy), which then hold for every output array
        (tests); by default new compact arrays.  Returns {name: array} of the detrended fields."""
        m = self._met_struct(met)
        o = MphipDetrend(float(met_detrend))
        mo = MphipRegridOut()
        mo.sx, mo.sy = out_strides or (met.ny * met.np, met.np)
        mo.sx2 = met.ny
        names = DETREND_FIELDS if fields is None else tuple(fields)
        if any(f not in FIELDS_3D for f in names):
            raise TypeError(f"unknown fields {sorted(set(names) - set(FIELDS_3D))}")
        res = {}
        for f in names:
            if out is not None and f in out:
                a = out[f]
            elif f in met.f3:
                a = np.empty((met.nx, met.ny, met.np), dtype=np.float32)
            else:
                continue
            _name_out(mo, f, a, (met.nx, met.ny, met.np), (4 * mo.sx, 4 * mo.sy, 4))
            if f in met.f3 and f in DETREND_FIELDS:
                res[f] = a
        for i, k in enumerate(FIELDS_3D):       # (a field that was not asked for is not passed: NULL on the input side too)
            if k in DETREND_FIELDS and k not in names:
                m.f3[i] = None
        self._chk(self.L.mphip_detrend_met(self.h, C.byref(m), C.byref(o), C.byref(mo)))
        return res

    # -- netCDF values to a met_t (mphip_ingest_met) ---------------------------
    def ingest_shape(self, axes, what):
        """nx2 of mphip_ingest_met for the axes of `axes` (lon, lat, p, coord_type) and the stages `what`: nx + 1 where the
        periodic column is added, else nx (mphip_ingest_shape; needs no device).  Raises where the call would refuse the
        grid or `what`."""
        m = self._met_struct(axes)
        n = C.c_int(0)
        if self.L.mphip_ingest_shape(C.byref(m), _bits(INGEST, what), C.byref(n)):
            raise MphipError("mphip_ingest_shape: the grid or `what` is refused")
        return n.value

    def ingest_met(self, *args, out=None, out_strides=None):
        """From a netCDF file's values to a met_t's on the device (mphip_ingest_met), in two forms.
        ingest_met(raw, axes, what): `raw` = {name: (array, dict(scale_factor=..., add_offset=..., fill=..., miss=...,
        scl=..., lnsp=...))} with the arrays in file order, float32 or int16 (packed), [nlev][ny][nx] or [ny][nx],
        C-contiguous (None: a descriptor without data, which the library refuses; `type` in the dict overrides the type
        the array's dtype gives); fill / miss are already of the stored type, 0 = none; `axes`: an object with lon, lat, p,
        coord_type (and nx, ny, np, npl) -- its f3 / f2, if any, are further inputs in met order.
        ingest_met(met, what): the met-order form, every field from met.f3 / met.f2 (the conventions of derive_met).
        `what`: names among decode, extrapolate, polar, periodic (or the OR of their MPHIP_INGEST_* bits).  `out`: {name:
        float32 array [nx2][ny][nlev] / [nx2][ny] to write into, or None to leave a field out} -- an input array itself
        for in-place use; views into larger arrays name their strides in floats as `out_strides` = (sx, sy, sx2), which
        then hold for every output array; by default new compact arrays.  Returns a Snapshot with nx2 longitudes."""
        if isinstance(args[0], dict):
            raw, met, what = args
        else:
            (met, what), raw = args, {}
        bits = _bits(INGEST, what)
        if not hasattr(met, "f3"):
            met = Snapshot(getattr(met, "time", 0.0), met.coord_type, met.lon, met.lat, met.p, {}, {})
        m = self._met_struct(met)
        if any(k in FIELDS_ML for k in list(raw) + list(met.f3)):
            m.npl = met.npl
        r = MphipIngestRaw()
        keep = []
        for name, (a, o) in raw.items():
            three = name in FIELDS_3D
            d = r.f3[FIELDS_3D.index(name)] if three else r.f2[FIELDS_2D.index(name)]
            o = dict(o)
            if a is not None:
                nlev = met.npl if name in FIELDS_ML else met.np
                assert a.dtype in (np.float32, np.int16) and a.flags["C_CONTIGUOUS"], name
                assert a.shape == ((nlev, met.ny, met.nx) if three else (met.ny, met.nx)), name
                keep.append(a)
                d.data = a.ctypes.data
            short = a is not None and a.dtype == np.int16
            d.type = int(o.pop("type", RAW_SHORT if short else RAW_FLOAT))
            d.lnsp = int(o.pop("lnsp", 0))
            d.scale_factor, d.add_offset = float(o.pop("scale_factor", 1.0)), float(o.pop("add_offset", 0.0))
            fill, miss = o.pop("fill", 0), o.pop("miss", 0)
            if short:
                d.fill_s, d.miss_s = int(fill), int(miss)
            else:
                d.fill_f, d.miss_f = float(fill), float(miss)
            d.scl = float(o.pop("scl", 1.0))
            if o:
                raise TypeError(f"unknown raw options {sorted(o)}")
        mo = MphipRegridOut()
        out = dict(out or {})
        n = C.c_int(0)
        if self.L.mphip_ingest_shape(C.byref(m), bits, C.byref(n)):
            self._shape_refused("ingest", mo, out, out_strides,
                                lambda: self.L.mphip_ingest_met(self.h, C.byref(m), C.byref(r), bits, C.byref(mo)))
        nx2 = n.value
        mo.sx, mo.sy, mo.sx2 = out_strides or (met.ny * max(met.np, m.npl), max(met.np, m.npl), met.ny)
        lon, lat, p = (np.empty(k, dtype=np.float64) for k in (nx2, met.ny, met.np))
        mo.lon, mo.lat, mo.p = _ptr(lon, _dp), _ptr(lat, _dp), _ptr(p, _dp)
        f3, f2 = {}, {}
        for f in FIELDS_3D:
            if f in out or f in raw or f in met.f3:
                nlev = met.npl if f in FIELDS_ML else met.np
                if f in out:
                    a = out[f]
                else:
                    a = np.empty((nx2, mo.sx // mo.sy, mo.sy), dtype=np.float32)[:, :met.ny, :nlev]
                if a is None:
                    continue
                _name_out(mo, f, a, (nx2, met.ny, nlev), (4 * mo.sx, 4 * mo.sy, 4))
                if f in raw or f in met.f3:
                    f3[f] = a
        for f in FIELDS_2D:
            if f in out or f in raw or f in met.f2:
                a = out[f] if f in out else np.empty((nx2, mo.sx2), dtype=np.float32)[:, :met.ny]
                if a is None:
                    continue
                _name_out(mo, f, a, (nx2, met.ny), (4 * mo.sx2, 4))
                if f in raw or f in met.f2:
                    f2[f] = a
        self._chk(self.L.mphip_ingest_met(self.h, C.byref(m), C.byref(r) if raw or bits & INGEST["decode"] else None, bits,
                                          C.byref(mo)))
        res = Snapshot(getattr(met, "time", 0.0), met.coord_type, lon, lat, p, f3, f2, out_strides)
        res.npl = met.npl
        return res

    # -- 16-bit packed level fields (MET_TYPE 2) ------------------------------
    def _met_packed_struct(self, met, packed):
        """mphip_met_packed_t of a snapshot `met` (axes, surface fields, the level fields that stay float) and `packed`:
        {name: (codes, scl, off[, lo, hi])} -- codes uint16 [nx][ny][nlev], C-contiguous (a view that starts anywhere in a
        larger array will do), scl / off float64 [nlev] (None: not given, which the library refuses); the limits default
        to PACK_LIMITS, those of the reader of the binary files."""
        m = MphipMetPacked()
        m.base = self._met_struct(met)
        if any(k in FIELDS_ML for k in packed):
            m.base.npl = met.npl
        for name, rec in packed.items():
            i = FIELDS_3D.index(name)
            q, scl, off = rec[:3]
            nlev = met.npl if name in FIELDS_ML else met.np
            assert q.dtype == np.uint16 and q.shape == (met.nx, met.ny, nlev) and q.flags["C_CONTIGUOUS"], name
            m.q3[i] = _ptr(q, _up)
            for slot, a in ((m.scl, scl), (m.off, off)):
                if a is not None:
                    assert a.dtype == np.float64 and a.shape == (nlev,) and a.flags["C_CONTIGUOUS"], name
                    slot[i] = _ptr(a, _dp)
            m.lo[i], m.hi[i] = rec[3:5] if len(rec) > 3 else PACK_LIMITS.get(name, PACK_LIMITS_OPEN)
        return m

    def update_met_packed(self, slot, met, packed):
        """set_met for a snapshot whose fields `packed` go to the device as codes and are decoded there
        (mphip_update_met_packed; the conventions of _met_packed_struct)."""
        m = self._met_packed_struct(met, packed)
        self._chk(self.L.mphip_update_met_packed(self.h, slot, C.byref(m)))
        self._mets[slot] = met

    def prefetch_met_packed(self, next_met, packed):
        """prefetch_met for such a snapshot (mphip_prefetch_met_packed); its arrays, the codes, scales and offsets
        included, must stay untouched until commit_met()."""
        m = self._met_packed_struct(next_met, packed)
        self._chk(self.L.mphip_prefetch_met_packed(self.h, C.byref(m)))
        self._next_met = next_met
        self._next_packed = packed

    def unpack_met(self, met, packed, out=None, out_strides=None):
        """Decode the fields `packed` on the device into float arrays (mphip_unpack_met).  `met`: the snapshot the codes
        belong to (its extents; its own fields are not read).  `out`: {name: float32 array [nx][ny][nlev] to write into}
        -- views into larger arrays name their strides in floats as `out_strides` = (sx, sy), which then hold for every
        output array; by default new compact arrays for every packed field.  Returns {name: array}."""
        m = self._met_packed_struct(met, packed)
        mo = MphipMet()
        mo.nx, mo.ny, mo.np, mo.npl = met.nx, met.ny, met.np, m.base.npl
        res = {}
        for name in (packed if out is None else out):
            nlev = met.npl if name in FIELDS_ML else met.np
            a = np.empty((met.nx, met.ny, nlev), dtype=np.float32) if out is None else out[name]
            sx, sy = out_strides or (met.ny * nlev, nlev)
            _name_out(mo, name, a, (met.nx, met.ny, nlev), (4 * sx, 4 * sy, 4))
            if name in FIELDS_ML:
                mo.sx_ml, mo.sy_ml = sx, sy
            else:
                mo.sx, mo.sy = sx, sy
            res[name] = a
        mo.sx2 = met.ny
        self._chk(self.L.mphip_unpack_met(self.h, C.byref(m), C.byref(mo)))
        return res

    def pack_met(self, met, fields=None, out=None):
        """Encode level fields of `met` (a snapshot with the conventions of derive_met) on the device
        (mphip_pack_met).  `fields`: the names to encode (default: every level field the snapshot has).  `out`: {name:
        (codes, scl, off)} arrays to write into (codes uint16 [nx][ny][nlev] C-contiguous, scl / off float64 [nlev] or
        None); by default new arrays.  Returns {name: (codes, scl, off)}."""
        m = self._met_struct(met)
        names = tuple(met.f3) if fields is None else tuple(fields)
        if any(k in FIELDS_ML for k in names):
            m.npl = met.npl
        for i, k in enumerate(FIELDS_3D):       # (a field that was not asked for is not passed)
            if k not in names:
                m.f3[i] = None
        out = dict(out or {})
        packed = {}
        for name in set(names) | set(out):
            nlev = met.npl if name in FIELDS_ML else met.np
            packed[name] = out.get(name) or (np.empty((met.nx, met.ny, nlev), dtype=np.uint16), np.empty(nlev), np.empty(nlev))
        empty = Snapshot(met.time, met.coord_type, met.lon, met.lat, met.p, {}, {})
        empty.npl = met.npl
        mo = self._met_packed_struct(empty, packed)
        self._chk(self.L.mphip_pack_met(self.h, C.byref(m), C.byref(mo)))
        return {k: packed[k] for k in names if k in met.f3}

    def set_met(self, slot, met):
        m = self._met_struct(met)
        self._chk(self.L.mphip_update_met(self.h, slot, C.byref(m)))
        self._mets[slot] = met

    def swap_met(self, new_met1):
        """mptrac_get_met when t passes met1: pointer swap, then read the next
        snapshot into met1 (src/mptrac.c:6486-6499)."""
        self._chk(self.L.mphip_swap_met(self.h))
        self._mets[0] = self._mets[1]
        self.set_met(1, new_met1)

    def swap_met_backward(self, new_met0):
        """mptrac_get_met when a backward run moves before met0: pointer swap (the old met0 is the new met1), then
        read the earlier snapshot into met0 -- mphip_swap_met + mphip_update_met on slot 0 of a running context; the
        sort and interpolation axes become the uploaded snapshot's."""
        self._chk(self.L.mphip_swap_met(self.h))
        self._mets[1] = self._mets[0]
        self.set_met(0, new_met0)

    def prefetch_met(self, next_met):
        """Start the upload of the snapshot after met1 beside the time steps
        (copy stream); its arrays must stay untouched until commit_met()."""
        m = self._met_struct(next_met)
        self._chk(self.L.mphip_prefetch_met(self.h, C.byref(m)))
        self._next_met = next_met

    def commit_met(self):
        """met1 -> met0, prefetched snapshot -> met1 (no host wait)."""
        self._chk(self.L.mphip_commit_met(self.h))
        self._mets[0] = self._mets[1]
        self._mets[1] = self._next_met
        self._next_met = None

    def discard_prefetch(self):
        self._chk(self.L.mphip_discard_prefetch(self.h))
        self._next_met = None

    def prefetch_done(self):
        return bool(self.L.mphip_prefetch_done(self.h))

    def intpol_met(self, time, p, lon, lat, fields):
        """The resident meteo pair interpolated at the caller's points (mphip_intpol_met: intpol_met_time_3d / _2d of the
        reference, its doubles bit for bit in both libraries).  `fields`: names of FIELDS_3D (pressure-level fields) and
        FIELDS_2D (surface fields), any order, repeats allowed; a scalar `time` holds for all points; `p` may be None
        when only surface fields are asked for.  Returns {name: float64 array [n]} (a name given twice: its last row)."""
        return dict(zip(fields, self.intpol_met_rows(time, p, lon, lat, fields)))

    def intpol_met_rows(self, time, p, lon, lat, fields, out=None):
        """intpol_met as the array [nfield][n], rows in the order of `fields` (`out`: such an array to write into)."""
        lon, lat = (np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64) for a in (lon, lat))
        n = len(lon)
        time = np.ascontiguousarray(np.atleast_1d(time), dtype=np.float64)
        if np.ndim(p) == 0 and p is not None:
            p = np.full(n, p)
        p = None if p is None else np.ascontiguousarray(p, dtype=np.float64)
        assert len(lat) == n and (p is None or len(p) == n)
        ids = (C.c_int * max(len(fields), 1))()
        for k, name in enumerate(fields):
            if name in FIELDS_2D:
                ids[k] = INTPOL_2D | FIELDS_2D.index(name)
            elif name in FIELDS_3D:
                ids[k] = FIELDS_3D.index(name)
            else:
                raise TypeError(f"unknown field {name}")
        if out is None:
            out = np.empty((len(fields), n), dtype=np.float64)
        assert out.dtype == np.float64 and out.shape == (len(fields), n) and out.flags["C_CONTIGUOUS"]
        self._chk(self.L.mphip_intpol_met(self.h, n, _ptr(time, _dp), len(time), None if p is None else _ptr(p, _dp),
                                          _ptr(lon, _dp), _ptr(lat, _dp), len(fields), ids, _ptr(out, _dp)))
        return out

    def update_atm(self, atm):
        sl = slice(0, self.n) if self.atm_is_local else slice(self.lo, self.hi)
        arrs = [np.ascontiguousarray(atm[k][sl], dtype=np.float64) for k in ("time", "p", "lon", "lat")]
        assert all(len(a) == self.n for a in arrs)
        q = np.asarray(atm["q"], dtype=np.float64)
        q = q.reshape(-1, q.shape[-1]) if q.size else np.zeros((self.nq, 0))
        q = np.ascontiguousarray(q[:self.nq, sl])
        qp = (_dp * NQ_MAX)()
        for iq in range(self.nq):
            qp[iq] = _ptr(q[iq], _dp)
        self._chk(self.L.mphip_update_atm(self.h, self.n, self.lo, self.n_total, self.nq,
                                          *[_ptr(a, _dp) for a in arrs], qp))

    def update_quantity(self, iq, values):
        """One quantity array in the caller's order (mphip_update_quantity)."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        assert v.shape == (self.n,)
        self._chk(self.L.mphip_update_quantity(self.h, int(iq), _ptr(v, _dp)))

    def replace_particles(self, atm):
        """A new particle set (any count) in the same context: what a C caller does when it hands a different
        atm_t to mptrac_update_device."""
        self.atm_is_local = False
        self.n_total = len(atm["time"])
        self.lo, self.hi = 0, self.n_total
        self.n = self.n_total
        self.update_atm(atm)

    # -- mptrac_update_host ---------------------------------------------------
    def get_atm(self, out=None):
        """Particle arrays in the caller's order; `out` = a dict returned earlier, to download into the
        same host arrays again (what a C caller's persistent atm_t does)."""
        if out is None:
            out = {k: np.empty(self.n) for k in ("time", "p", "lon", "lat")}
            out["q"] = np.empty((self.nq, self.n))
        q = out["q"]
        qp = (_dp * NQ_MAX)()
        for iq in range(self.nq):
            qp[iq] = _ptr(q[iq], _dp)
        self._chk(self.L.mphip_get_atm(self.h, _ptr(out["time"], _dp), _ptr(out["p"], _dp),
                                       _ptr(out["lon"], _dp), _ptr(out["lat"], _dp), qp))
        out["q"] = q
        return out

    def get_cache(self):
        uvwp = np.empty((self.n, 3), dtype=np.float32)
        dt = np.empty(self.n)
        ctr = C.c_uint64()
        self._chk(self.L.mphip_get_cache(self.h, _ptr(uvwp, _fp), _ptr(dt, _dp), C.byref(ctr)))
        return {"uvwp": uvwp, "dt": dt, "rng_ctr": ctr.value}

    def state(self):
        s = self.get_atm()
        s["uvwp"] = self.get_cache()["uvwp"]
        return s

    def set_balloon(self, ts, ps):
        """The pressure time series module_isosurf_init reads for ISOSURF 4
        (src/mptrac.c:4925-4951)."""
        ts = np.ascontiguousarray(ts, dtype=np.float64)
        ps = np.ascontiguousarray(ps, dtype=np.float64)
        self._chk(self.L.mphip_update_iso(self.h, None, _ptr(ts, _dp), _ptr(ps, _dp), len(ts)))

    def get_iso(self):
        iso = np.empty(self.n)
        self._chk(self.L.mphip_get_iso(self.h, _ptr(iso, _dp)))
        return iso

    # -- stepping -------------------------------------------------------------
    def timesteps_init(self, tmin, tmax):
        """module_timesteps_init (src/mptrac.c:6046-6073) -- host logic on the
        global minimum / maximum particle time."""
        c = self.ctl
        c.t_start, c.t_stop = timestep_range(c.direction, c.dt_mod, c.t_stop, tmin, tmax)
        self.update_ctl()

    def run_timestep(self, t):
        self._chk(self.L.mphip_run_timestep(self.h, t))

    def module(self, name, t=0.0):
        self._chk(self.L.mphip_module(self.h, MOD[name], t))

    def sort(self):
        self._chk(self.L.mphip_module(self.h, MOD["sort"], 0.0))
        keys = np.empty(self.n)
        perm = np.empty(self.n, dtype=np.int32)
        self._chk(self.L.mphip_get_sort(self.h, _ptr(keys, _dp), _ptr(perm, C.POINTER(C.c_int))))
        return keys, perm

    def get_sort(self):
        """Sorted keys and permutation of the last module_sort (mphip_get_sort), without sorting again."""
        keys = np.empty(self.n)
        perm = np.empty(self.n, dtype=np.int32)
        self._chk(self.L.mphip_get_sort(self.h, _ptr(keys, _dp), _ptr(perm, C.POINTER(C.c_int))))
        return keys, perm

    def sort_counts(self):
        """(module_sort calls answered by the repair of the previous order, calls sorted from scratch) of this context"""
        return self._sort_counts()[:2]

    def sorts_undone(self):
        """module_sort calls that found the particles in the internal locality order and restored the caller's first"""
        return self._sort_counts()[2]

    def _sort_counts(self):
        if not hasattr(self.L, "mphip_get_sort_counts"):
            raise MphipError(f"{self.L._name} has no mphip_get_sort_counts: the library was built before the sort counters")
        repaired, scratch, undone = C.c_longlong(), C.c_longlong(), C.c_longlong()
        self._chk(self.L.mphip_get_sort_counts(self.h, C.byref(repaired), C.byref(scratch), C.byref(undone)))
        return repaired.value, scratch.value, undone.value

    def grid_sums(self, t, out=None):
        """Counts, sums of q and of q^2 per output cell (mphip_grid_sums).  `out` = (cnt, mean, sigma) of an
        earlier call: the arrays are filled again instead of allocated (a caller that writes one output after the
        other, like write_grid with its own buffers)."""
        ncell = self.ctl.grid_nx * self.ctl.grid_ny * self.ctl.grid_nz
        if out is not None:
            cnt, mean, sigma = out
            assert cnt.shape == (ncell,) and mean.shape == (self.nq, ncell) and sigma.shape == (self.nq, ncell)
        else:
            cnt = np.zeros(ncell, dtype=np.int32)
            mean = np.zeros((self.nq, ncell))
            sigma = np.zeros((self.nq, ncell))
        self._chk(self.L.mphip_grid_sums(self.h, t, _ptr(cnt, C.POINTER(C.c_int)), _ptr(mean, _dp),
                                         _ptr(sigma, _dp)))
        return cnt, mean, sigma

    def set_grid_kernel(self, kz=(), kw=()):
        """Vertical weighting function of the gridded output (GRID_KERNEL); no nodes: off."""
        kz = np.ascontiguousarray(kz, dtype=np.float64)
        kw = np.ascontiguousarray(kw, dtype=np.float64)
        assert kz.shape == kw.shape
        self._chk(self.L.mphip_set_grid_kernel(self.h, len(kz), _ptr(kz, _dp), _ptr(kw, _dp)))

    # -- the particle loops of write_csi / write_prof / write_sample / write_station -----------------------------
    @staticmethod
    def _kernel_fn(kernel):
        kz, kw = (np.ascontiguousarray(a, dtype=np.float64) for a in (kernel if kernel is not None else ((), ())))
        assert kz.shape == kw.shape
        return kz, kw

    def box_sums(self, box, t, qnt, nmember=1, qnt_member=-1, kernel=None):
        """sum[nmember][nx * ny * nz] of kernel_weight * q[qnt] over the particles of the time step around t
        (mphip_box_sums).  `box` = (lon0, lon1, nx, lat0, lat1, ny, z0, z1, nz), `kernel` = (kz, kw) or None."""
        b = MphipBox(*box)
        kz, kw = self._kernel_fn(kernel)
        out = np.zeros((nmember, b.nx * b.ny * b.nz))
        self._chk(self.L.mphip_box_sums(self.h, C.byref(b), t, qnt, nmember, qnt_member, len(kz), _ptr(kz, _dp), _ptr(kw, _dp),
                                        _ptr(out, _dp)))
        return out

    def sample_obs(self, t0, t1, lon, lat, z, dx, dz=0.0, kernel=None):
        """(count, mass) per observation: the particles inside the cylinder of radius dx [km] (half depth dz [km] if
        positive) around it with t0 <= time <= t1, and their kernel-weighted mass (mphip_sample_obs)."""
        lon, lat, z = (np.ascontiguousarray(a, dtype=np.float64) for a in (lon, lat, z))
        assert lon.shape == lat.shape == z.shape
        kz, kw = self._kernel_fn(kernel)
        count = np.zeros(len(lon), dtype=np.int32)
        mass = np.zeros(len(lon))
        self._chk(self.L.mphip_sample_obs(self.h, t0, t1, len(lon), _ptr(lon, _dp), _ptr(lat, _dp), _ptr(z, _dp), dx, dz,
                                          len(kz), _ptr(kz, _dp), _ptr(kw, _dp), _ptr(count, C.POINTER(C.c_int)), _ptr(mass, _dp)))
        return count, mass

    def station_hits(self, t, lon, lat, r, stat_t0, stat_t1, qnt_stat=-1, cap=1024):
        """(nhit, index, rows[nhit][4 + nq]) of the particles write_station would list (mphip_station_hits); with
        nhit > cap nothing was listed and no flag was set: (nhit, None, None)."""
        n = C.c_int(0)
        index = np.zeros(max(cap, 1), dtype=np.int32)
        rows = np.zeros((max(cap, 1), 4 + self.nq))
        self._chk(self.L.mphip_station_hits(self.h, t, lon, lat, r, stat_t0, stat_t1, qnt_stat, cap, C.byref(n),
                                            _ptr(index, C.POINTER(C.c_int)), _ptr(rows, _dp)))
        if n.value > cap:
            return n.value, None, None
        return n.value, index[:n.value].copy(), rows[:n.value].copy()

    def select_atm(self, stride=1, first=0, last=-1, time=None, z=None, lon=None, lat=None, near=None,
                   rows=("time", "p", "lon", "lat", "q"), cap=None):
        """The particles with external index first, first + stride, ... <= last that no given criterion rejects, in
        ascending index, without downloading the others (mphip_select_atm).  `time`, `z`, `lon`, `lat`: (lo, hi) or None;
        `near`: (lon, lat, r_km).  Returns {"n", "index", the requested rows cut to n, "q" of shape (nq, n)}; `rows` names
        the rows wanted ("q": all quantities, or "q0", "q1", ... for single ones -- the others stay NaN in "q").
        cap=None: the number of candidates, which always suffices; an explicit cap below n: {"n": n} with None for the
        rows, and nothing was copied."""
        s = MphipSelect()
        s.first, s.last, s.stride = int(first), int(last), int(stride)
        for name, pair, lo, hi in (("time", time, "t0", "t1"), ("z", z, "z0", "z1"), ("lon", lon, "lon0", "lon1"),
                                   ("lat", lat, "lat0", "lat1")):
            if pair is not None:
                setattr(s, "use_" + name, 1)
                setattr(s, lo, float(pair[0]))
                setattr(s, hi, float(pair[1]))
        if near is not None:
            s.use_near = 1
            s.near_lon, s.near_lat, s.near_r = (float(v) for v in near)
        if cap is None:
            end = self.n - 1 if last < 0 or last >= self.n else int(last)
            cap = (end - int(first)) // int(stride) + 1 if stride >= 1 and 0 <= first <= end else 0
        cap = int(cap)
        m = max(cap, 1)
        rows = tuple(rows)
        unknown = [r for r in rows if r not in ("index", "time", "p", "lon", "lat", "q")
                   and not (r[:1] == "q" and r[1:].isdigit() and int(r[1:]) < self.nq)]
        if unknown:
            raise KeyError(f"not a row of select_atm: {unknown}")
        want_q = [("q" in rows or f"q{iq}" in rows) for iq in range(self.nq)]
        out = {k: np.empty(m) for k in ("time", "p", "lon", "lat") if k in rows}
        index = np.empty(m, dtype=np.int32)
        q = np.full((self.nq, m), np.nan) if any(want_q) else None
        qp = (_dp * NQ_MAX)()
        for iq in range(self.nq):
            if want_q[iq]:
                qp[iq] = _ptr(q[iq], _dp)
        n = C.c_longlong(0)
        ptr = {k: (_ptr(out[k], _dp) if k in out else None) for k in ("time", "p", "lon", "lat")}
        self._chk(self.L.mphip_select_atm(self.h, C.byref(s), cap, C.byref(n), _ptr(index, C.POINTER(C.c_int)), ptr["time"],
                                          ptr["p"], ptr["lon"], ptr["lat"], qp if q is not None else None))
        res = {"n": n.value}
        if n.value > cap:
            res.update({k: None for k in ("index", *out)})
            if q is not None:
                res["q"] = None
            return res
        res["index"] = index[:n.value].copy()
        for k, v in out.items():
            res[k] = v[:n.value].copy()
        if q is not None:
            res["q"] = q[:, :n.value].copy()
        return res

    def set_radio_decay(self, quantities, on=True):
        """module_radio_decay (mphip_set_radio_decay).  `quantities`: the quantity names of the particles (in quantity
        order, as given to ctl_from_quantities; the activities among them are found by name), {activity name: index},
        or the MPHIP_NRADIO indices in RADIO_ACTIVITIES order (-1: absent).  on=False: the time step leaves the
        activities alone (module_mixing still mixes them)."""
        if isinstance(quantities, dict):
            unknown = set(quantities) - set(RADIO_ACTIVITIES)
            if unknown:
                raise KeyError(f"not an activity: {sorted(unknown)}")
            idx = [int(quantities.get(n, -1)) for n in RADIO_ACTIVITIES]
        else:
            quantities = list(quantities)
            if any(isinstance(q, str) for q in quantities):
                idx = list(radio_from_quantities(quantities))
            else:
                if len(quantities) != len(RADIO_ACTIVITIES):
                    raise ValueError(f"{len(RADIO_ACTIVITIES)} activity indices expected, got {len(quantities)}")
                idx = [int(q) for q in quantities]
        arr = (C.c_int * len(RADIO_ACTIVITIES))(*idx)
        self._chk(self.L.mphip_set_radio_decay(self.h, 1 if on else 0, arr))

    def set_radio_depo(self, grid, on=True):
        """module_radio_depo (mphip_set_radio_depo): `grid` = (lon0, lon1, nx, lat0, lat1, ny) of the ground grid -- or the
        nine numbers of a box as box_sums takes them, with nz = 1 --, None with on=False: only the switch.  A new grid
        starts a new, empty inventory; the same grid keeps it."""
        if grid is None:
            self._chk(self.L.mphip_set_radio_depo(self.h, 1 if on else 0, None))
            return
        grid = tuple(grid)
        if len(grid) == 6:
            grid = grid + (0.0, 1.0, 1)
        b = MphipBox(*grid)
        self._chk(self.L.mphip_set_radio_depo(self.h, 1 if on else 0, C.byref(b)))
        self._radio_depo_cells = b.nx * b.ny + 1

    def radio_depo(self):
        """(t_inv, wet, dry) of the ground inventory (mphip_get_radio_depo): wet, dry [activity in RADIO_ACTIVITIES order]
        [nx * ny + 1] in Bq, cell ix * ny + iy, the last element of a row = deposited outside the grid; t_inv is NaN
        before the first step.  Summed over the ranks."""
        n = getattr(self, "_radio_depo_cells", 1)
        wet = np.zeros((len(RADIO_ACTIVITIES), n))
        dry = np.zeros((len(RADIO_ACTIVITIES), n))
        t_inv = C.c_double(0.0)
        self._chk(self.L.mphip_get_radio_depo(self.h, C.byref(t_inv), _ptr(wet, _dp), _ptr(dry, _dp)))
        return t_inv.value, wet, dry

    def shortcuts(self):
        """{"ps", "pct", "turb", "conv"}: the bounds of the four early exits (mphip_get_shortcuts); -inf = never taken"""
        b = (C.c_double * 4)()
        self._chk(self.L.mphip_get_shortcuts(self.h, b))
        return dict(zip(("ps", "pct", "turb", "conv"), (float(v) for v in b)))

    def synchronize(self):
        self._chk(self.L.mphip_synchronize(self.h))

    def run_timesteps(self, t_first, nsteps):
        """nsteps consecutive time steps starting at t_first (mphip_run_timesteps)."""
        self._chk(self.L.mphip_run_timesteps(self.h, float(t_first), int(nsteps)))

    def set_option(self, name, value):
        self._chk(self.L.mphip_set_option(self.h, name.encode(), float(value)))

    def set_allreduce(self, fn):
        """fn(device_pointer:int, count:int) -> None; sums `count` doubles at
        that device address over all ranks."""
        def _cb(ptr, count, _user):
            try:
                fn(ptr, count)
                return 0
            except Exception as e:   # surfaced as an error code to the C side
                print("allreduce hook failed:", e)
                return 1
        self._cb = ALLREDUCE_FN(_cb)
        self._chk(self.L.mphip_set_allreduce(self.h, self._cb, None))

    @staticmethod
    def comm_unique_id():
        """128-byte RCCL identifier (created on rank 0, handed to the other ranks by the host)."""
        buf = C.create_string_buffer(128)
        if load().mphip_comm_unique_id(buf):
            raise MphipError("mphip_comm_unique_id failed (librccl not loadable?)")
        return buf.raw

    def comm_init(self, nranks, rank, unique_id):
        """RCCL communicator of this context: the gridded reductions become all-reduces on its stream."""
        self._chk(self.L.mphip_comm_init(self.h, int(nranks), int(rank), C.c_char_p(bytes(unique_id))))

    def comm_destroy(self):
        self._chk(self.L.mphip_comm_destroy(self.h))

    def comm_query(self):
        """(ranks, rank) as the RCCL communicator reports them; (0, 0) without one."""
        n, r = C.c_int(), C.c_int()
        self._chk(self.L.mphip_comm_query(self.h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def profile_begin(self):
        self._chk(self.L.mphip_profile_begin(self.h))

    def profile_end(self):
        n = C.c_longlong()
        ms = C.c_double()
        self._chk(self.L.mphip_profile_end(self.h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    # -- device self tests ------------------------------------------------------
    def test_sincosf(self, first_bits, count):
        c = np.empty(count, dtype=np.float32)
        s = np.empty(count, dtype=np.float32)
        self._chk(self.L.mphip_test_sincosf(self.h, first_bits, count, _ptr(c, _fp), _ptr(s, _fp)))
        return c, s

    def test_piece(self, piece, reps=1):
        """Profiling aid (tools/piece_cost.py): run one building block of the step kernel per particle."""
        chk = C.c_double(0.0)
        self._chk(self.L.mphip_test_piece(self.h, int(piece), int(reps), C.byref(chk)))
        return chk.value

    def test_meso_table(self, shape):
        """module_diff_meso's wind deviations per raw cell of the current meteo pair, [nx - 1][ny - 1][np - 1][3], as the
        lean kernels read them (shape: the grid's (nx, ny, np))."""
        nx, ny, npl = shape
        out = np.empty((nx - 1, ny - 1, npl - 1, 3), dtype=np.float32)
        self._chk(self.L.mphip_test_meso_table(self.h, _ptr(out, _fp), out.size // 3))
        return out

    def test_rng(self, ctr, n, method):
        out = np.empty(n)
        self._chk(self.L.mphip_test_rng(self.h, ctr, n, method, _ptr(out, _dp)))
        return out

    def test_libm(self, fn, x, y=None, lds=False):
        """exp / log / pow / sqrt of the arrays as the kernels evaluate them (mphip_libm.h; tables from LDS if asked)."""
        op = {"exp": 0, "log": 1, "pow": 2, "sqrt": 3, "cos": 4, "sin": 5, "cos_wide": 6, "sin_wide": 7}[fn] + (16 if lds else 0)
        x = np.ascontiguousarray(x, dtype=np.float64)
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.float64)
        out = np.empty_like(x)
        self._chk(self.L.mphip_test_libm(self.h, op, _ptr(x, _dp), _ptr(y, _dp) if y is not None else None, len(x), _ptr(out, _dp)))
        return out
