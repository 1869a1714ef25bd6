/*
 * mptrac_hip.h -- C ABI of the MI355X (gfx950) back end for MPTRAC's
 * per-particle time-step loop.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or framework
 * types.  Each entry point names the reference interface it stands in for
 * (paths relative to the reference repository; mptrac.c = src/mptrac.c,
 * mptrac.h = src/mptrac.h).  INTEGRATION.md shows the few lines a maintainer
 * adds to mptrac.c to route the OpenACC data/compute regions through it.
 *
 * Residency contract (same as the reference's OpenACC build, mptrac.c:8005-8113,
 * 8248-8255): after mphip_update_atm() the device copy of the particles is
 * authoritative; the host sees it again only through mphip_get_atm().
 *
 * Error convention: every int-returning call returns 0 on success and a
 * non-zero code otherwise; mphip_last_error() gives the text.  The reference
 * has no error returns on this path (ERRMSG prints and exits,
 * mptrac.h:2406-2410); a host mirroring that behaviour prints the text and
 * calls exit(EXIT_FAILURE).  There is no CPU fallback: without a usable HIP
 * device mphip_create() fails.
 */
#ifndef MPTRAC_HIP_H
#define MPTRAC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPHIP_NQ_MAX 16

/* 3-D meteo fields (met_t, mptrac.h:3962-4012), float [ix][iy][ip] */
enum { MPHIP_U = 0, MPHIP_V, MPHIP_W, MPHIP_T, MPHIP_LWC, MPHIP_RWC, MPHIP_IWC, MPHIP_SWC,
       /* model-level fields (met_t pl, ul, vl, zetal, zeta_dotl; mptrac.h:3997-4012), float [ix][iy][npl] */
       MPHIP_PL, MPHIP_UL, MPHIP_VL, MPHIP_ZETAL, MPHIP_ZETA_DOTL,
       MPHIP_H2O,   /* water vapour on pressure levels (module_diff_pbl, module_meteo) */
       /* read by module_meteo only (INTPOL_TIME_ALL, mptrac.h:1278-1318) */
       MPHIP_Z, MPHIP_PV, MPHIP_O3, MPHIP_CC,
       MPHIP_WL,    /* vertical velocity on model levels (met_t wl), float [ix][iy][npl]: ADVECT_VERT_COORD 2 */
       MPHIP_N3D };
/* 2-D meteo fields (met_t, mptrac.h:3886-3958), float [ix][iy] */
enum { MPHIP_PS = 0, MPHIP_PBL, MPHIP_CAPE, MPHIP_CIN, MPHIP_PEL, MPHIP_PCT, MPHIP_PCB, MPHIP_CL,
       MPHIP_ESS, MPHIP_NSS, MPHIP_SHF,   /* surface stresses and sensible heat flux (module_diff_pbl) */
       /* read by module_meteo only */
       MPHIP_TS, MPHIP_ZS, MPHIP_US, MPHIP_VS, MPHIP_LSM, MPHIP_SST, MPHIP_PT, MPHIP_TT, MPHIP_ZT, MPHIP_H2OT,
       MPHIP_PLCL, MPHIP_PLFC, MPHIP_O3C,
       MPHIP_N2D };

/* Quantities module_meteo fills (SET_ATM list, mptrac.c:5091-5157, in that order); mphip_ctl_t::qnt_met[k]
 * is the reference's ctl->qnt_<name> (-1 = not requested).  The last seven come from the zonal-mean
 * climatologies of clim_t (mphip_update_clim_zm): hno3, oh, h2o2, ho2, o1d = clim_zm / clim_oh at the particle,
 * tnat = nat_temperature(p, h2o, hno3), tsts = (tice + tnat) / 2 (needs both, mptrac.c:5074-5076).  The
 * self-assignments of the list (zeta, zeta_dot, eta, eta_dot) have no entry. */
enum { MPHIP_MQ_PS = 0, MPHIP_MQ_TS, MPHIP_MQ_ZS, MPHIP_MQ_US, MPHIP_MQ_VS, MPHIP_MQ_ESS, MPHIP_MQ_NSS,
       MPHIP_MQ_SHF, MPHIP_MQ_LSM, MPHIP_MQ_SST, MPHIP_MQ_PBL, MPHIP_MQ_PT, MPHIP_MQ_TT, MPHIP_MQ_ZT,
       MPHIP_MQ_H2OT, MPHIP_MQ_ZG, MPHIP_MQ_P, MPHIP_MQ_T, MPHIP_MQ_RHO, MPHIP_MQ_U, MPHIP_MQ_V, MPHIP_MQ_W,
       MPHIP_MQ_H2O, MPHIP_MQ_O3, MPHIP_MQ_LWC, MPHIP_MQ_RWC, MPHIP_MQ_IWC, MPHIP_MQ_SWC, MPHIP_MQ_CC,
       MPHIP_MQ_PCT, MPHIP_MQ_PCB, MPHIP_MQ_CL, MPHIP_MQ_PLCL, MPHIP_MQ_PLFC, MPHIP_MQ_PEL, MPHIP_MQ_CAPE,
       MPHIP_MQ_CIN, MPHIP_MQ_O3C, MPHIP_MQ_VH, MPHIP_MQ_VZ, MPHIP_MQ_PSAT, MPHIP_MQ_PSICE, MPHIP_MQ_PW,
       MPHIP_MQ_SH, MPHIP_MQ_RH, MPHIP_MQ_RHICE, MPHIP_MQ_THETA, MPHIP_MQ_ZETA_D, MPHIP_MQ_TVIRT,
       MPHIP_MQ_LAPSE, MPHIP_MQ_PV, MPHIP_MQ_TDEW, MPHIP_MQ_TICE,
       MPHIP_MQ_HNO3, MPHIP_MQ_OH, MPHIP_MQ_H2O2, MPHIP_MQ_HO2, MPHIP_MQ_O1D, MPHIP_MQ_TNAT, MPHIP_MQ_TSTS,
       MPHIP_NMQ };

/* Zonal-mean climatologies of clim_t that module_meteo samples (clim_zm_t members hno3, oh, h2o2, ho2, o1d,
 * mptrac.h:3745-3776, 3805-3817) */
enum { MPHIP_ZM_HNO3 = 0, MPHIP_ZM_OH, MPHIP_ZM_H2O2, MPHIP_ZM_HO2, MPHIP_ZM_O1D, MPHIP_NZM };

/* Trace gases module_bound_cond sets from a surface time series and module_mixing mixes (clim_ts_t members ccl4,
 * ccl3f, ccl2f2, n2o, sf6 of clim_t, mptrac.h:3820-3832; quantities Cccl4, Cccl3f, Cccl2f2, Cn2o, Csf6) */
enum { MPHIP_TR_CCL4 = 0, MPHIP_TR_CCL3F, MPHIP_TR_CCL2F2, MPHIP_TR_N2O, MPHIP_TR_SF6, MPHIP_NTR };

/* Module bits for mphip_module(); one bit per reference module_* function
 * (declarations mptrac.h:6140-7205). */
enum {
  MPHIP_MOD_TIMESTEPS  = 1 << 0,   /* module_timesteps   mptrac.c:5999 */
  MPHIP_MOD_POSITION   = 1 << 1,   /* module_position    mptrac.c:5435 (first call, mptrac.c:7884) */
  MPHIP_MOD_ADVECT     = 1 << 2,   /* module_advect      mptrac.c:3598 */
  MPHIP_MOD_DIFF_TURB  = 1 << 3,   /* module_diff_turb   mptrac.c:4588 */
  MPHIP_MOD_DIFF_MESO  = 1 << 4,   /* module_diff_meso   mptrac.c:4266 */
  MPHIP_MOD_CONVECTION = 1 << 5,   /* module_convection  mptrac.c:4102 */
  MPHIP_MOD_SEDI       = 1 << 6,   /* module_sedi        mptrac.c:5859 */
  MPHIP_MOD_POSITION2  = 1 << 7,   /* module_position, second call (mptrac.c:7919) */
  MPHIP_MOD_LOSS_ZERO  = 1 << 8,   /* q[loss_rate] = 0   mptrac.c:7932-7936 */
  MPHIP_MOD_DECAY      = 1 << 9,   /* module_decay       mptrac.c:4227 */
  MPHIP_MOD_WET_DEPO   = 1 << 10,  /* module_wet_depo    mptrac.c:6155 */
  MPHIP_MOD_DRY_DEPO   = 1 << 11,  /* module_dry_depo    mptrac.c:4738 */
  MPHIP_MOD_ADVECT_INIT = 1 << 12, /* module_advect_init mptrac.c:3762 (not guarded by dt) */
  MPHIP_MOD_DIFF_PBL   = 1 << 13,  /* module_diff_pbl    mptrac.c:4343 (runs between diff_turb and diff_meso) */
  MPHIP_MOD_METEO      = 1 << 14,  /* module_meteo       mptrac.c:5062 (own kernel; not guarded by dt) */
  MPHIP_MOD_ISOSURF    = 1 << 15,  /* module_isosurf     mptrac.c:4956 (not guarded by dt; between sedi and position2) */
  MPHIP_MOD_SORT       = 1 << 16,  /* module_sort        mptrac.c:5887 (own kernels) */
  MPHIP_MOD_MIXING     = 1 << 17,  /* module_mixing      mptrac.c:5169 (own kernels) */
  MPHIP_MOD_BOUND_COND = 1 << 18,  /* module_bound_cond  mptrac.c:3789, first call (mptrac.c:7929) */
  MPHIP_MOD_BOUND_COND2 = 1 << 19, /* module_bound_cond, second call (mptrac.c:8000) */
  MPHIP_MOD_ISOSURF_INIT = 1 << 20, /* module_isosurf_init mptrac.c:4886, modes 1-3 (not guarded by dt) */
  MPHIP_MOD_OH_CHEM    = 1 << 21,  /* module_oh_chem     mptrac.c:5351-5434 (between module_mixing and module_wet_depo) */
  MPHIP_MOD_CHEM_GRID  = 1 << 22,  /* module_chem_grid   (own kernels; between module_mixing and module_oh_chem) */
  MPHIP_MOD_H2O2_CHEM  = 1 << 23,  /* module_h2o2_chem   (own kernel; between module_oh_chem and module_wet_depo) */
  MPHIP_MOD_TRACER_CHEM = 1 << 24, /* module_tracer_chem (own kernel; between module_h2o2_chem and module_wet_depo) */
  MPHIP_MOD_RADIO_DECAY = 1 << 25, /* module_radio_decay mptrac.c:5493-5572 (step kernel's tail; between
                                      module_tracer_chem and module_wet_depo; mphip_set_radio_decay) */
  MPHIP_MOD_RADIO_DEPO = 1 << 26   /* module_radio_depo (own kernels; behind the step's tail; mphip_set_radio_depo) */
};

/* Radionuclide activities of module_radio_decay and module_mixing (quantities Arn222, Apb210, Abe7, Acs137, Ai131,
 * Axe133 of the reference's SET_QNT table): slots of mphip_set_radio_decay's qnt[] */
enum { MPHIP_RN_RN222 = 0, MPHIP_RN_PB210, MPHIP_RN_BE7, MPHIP_RN_CS137, MPHIP_RN_I131, MPHIP_RN_XE133, MPHIP_NRADIO };

/* Hot-path subset of ctl_t (mptrac.h:2494-3553); same field names, meaning
 * and defaults as mptrac_read_ctl (mptrac.c:6723-7741).  A compact POD is
 * passed instead of the 469 kB reference struct. */
typedef struct {
  int direction;
  int met_coord_type;
  double t_start, t_stop, dt_mod, dt_met;
  double met_utm_ref_lat;
  int nq;
  int qnt_m, qnt_vmr, qnt_rp, qnt_rhop, qnt_ens;
  int qnt_loss_rate, qnt_mloss_decay, qnt_mloss_wet, qnt_mloss_dry;
  int qnt_zeta, qnt_eta;
  int nens;
  int advect;
  int advect_vert_coord;   /* 0 pressure levels, 1 zeta, 2 pressure with model-level winds (pl, ul, vl, wl), 3 eta (mptrac.c:3609-3757) */
  int rng_type;
  int diffusion;
  int turb_pbl_scheme;
  int conv_mix_pbl;
  double turb_dx_pbl, turb_dx_trop, turb_dx_strat;
  double turb_dz_pbl, turb_dz_trop, turb_dz_strat;
  double turb_mesox, turb_mesoz, turb_pbl_trans;
  double conv_pbl_trans, conv_cape, conv_cin, conv_dt;
  double sort_dt;
  double tdec_trop, tdec_strat;
  double mixing_dt, mixing_trop, mixing_strat;
  double mixing_z0, mixing_z1, mixing_lon0, mixing_lon1, mixing_lat0, mixing_lat1;
  int mixing_nx, mixing_ny, mixing_nz;
  int pad0;
  double wet_depo_pre[2];
  double wet_depo_ic_a, wet_depo_ic_b, wet_depo_bc_a, wet_depo_bc_b;
  double wet_depo_ic_h[2], wet_depo_bc_h[2];
  double wet_depo_so2_ph, wet_depo_ic_ret_ratio, wet_depo_bc_ret_ratio;
  double dry_depo_vdep, dry_depo_dp;
  double grid_z0, grid_z1, grid_lon0, grid_lon1, grid_lat0, grid_lat1;
  int grid_nx, grid_ny, grid_nz;
  int pad1;
  /* module_meteo (mptrac.c:7921-7924): runs when met_dt_out > 0 and (met_dt_out < dt_mod or
   * fmod(t, met_dt_out) == 0); reference default 0.1 (mptrac.c:7197) */
  double met_dt_out;
  int qnt_met[MPHIP_NMQ];
  /* module_isosurf (ISOSURF, mptrac.c:7208) and module_bound_cond (BOUND_*, mptrac.c:7266-7289) */
  int isosurf;            /* 0 none, 1 pressure, 2 density, 3 potential temperature, 4 balloon time series */
  int bound_pbl;
  int qnt_aoa;            /* age of air: set by module_bound_cond, mixed by module_mixing */
  int pad3;
  double bound_mass, bound_mass_trend, bound_vmr, bound_vmr_trend;
  double bound_lat0, bound_lat1, bound_p0, bound_p1, bound_dps, bound_dzs, bound_zetas;
  /* module_meteo's OH quantity (clim_oh, mptrac.c:89-120): exponent of the diurnal scaling (OH_CHEM_BETA, 0 = none)
   * and the reference longitude a Cartesian grid is centred on (MET_UTM_REF_LON) */
  double oh_chem_beta;
  double met_utm_ref_lon;
  /* ctl->qnt_Cccl4, qnt_Cccl3f, qnt_Cccl2f2, qnt_Cn2o, qnt_Csf6 (MPHIP_TR_* order; -1 = not present): mixed by
   * module_mixing (mptrac.c:5223-5230), set by module_bound_cond where a time series was uploaded
   * (mphip_update_clim_ts; mptrac.c:3857-3875) */
  int qnt_tracer[MPHIP_NTR];
  int pad4;
  /* module_oh_chem (OH_CHEM_REACTION, OH_CHEM[0..3] of mptrac_read_ctl; SPECIES presets, mptrac.c:7291-7383):
   * reaction type 0 (off) ... 3, its rate constants, and ctl->qnt_mloss_oh (-1 = not present).  Appended: every
   * earlier member keeps its offset. */
  int oh_chem_reaction;
  int qnt_mloss_oh;
  double oh_chem[4];
  /* module_h2o2_chem (H2O2_CHEM_REACTION: 0 off, else on; ctl->qnt_mloss_h2o2) and module_chem_grid (ctl->qnt_Cx,
   * MOLMASS, CHEMGRID_*), which runs when either chemistry is on and both m and Cx are present.  Appended: every
   * earlier member keeps its offset. */
  int h2o2_chem_reaction;
  int qnt_mloss_h2o2;
  int qnt_Cx;
  int chemgrid_nx, chemgrid_ny, chemgrid_nz;
  double molmass;
  double chemgrid_lon0, chemgrid_lon1, chemgrid_lat0, chemgrid_lat1, chemgrid_z0, chemgrid_z1;
  /* module_tracer_chem (TRACER_CHEM: 0 off, else on): loss of the quantities Cccl4, Cccl3f, Cccl2f2 and Cn2o of
   * qnt_tracer by photolysis (mphip_update_clim_photo) and reaction with O(1D) (the O1D zonal mean); Csf6 is kept.
   * Appended: every earlier member keeps its offset. */
  int tracer_chem;
  int pad5;
} mphip_ctl_t;

/* View of one met_t snapshot (mptrac.h:3844-4014).  The arrays stay where the
 * host has them; strides describe the reference's fixed-extent layout
 * (float u[EX][EY][EP]: sx = EY*EP, sy = EP; float ps[EX][EY]: sx2 = EY) or a
 * compact one (sx = ny*np, sy = np, sx2 = ny).  A NULL field is "not
 * provided"; modules that need it then fail with an error. */
typedef struct {
  double time;
  int coord_type;
  int nx, ny, np;
  int npl;                 /* number of model levels of the MPHIP_PL ... fields (0 = none) */
  const double *lon, *lat, *p;
  long long sx, sy, sx2;
  long long sx_ml, sy_ml;  /* strides of the model-level arrays (same as sx, sy for met_t's [EX][EY][EP]) */
  const float *f3[MPHIP_N3D];
  const float *f2[MPHIP_N2D];
} mphip_met_t;

typedef struct mphip_ctx mphip_ctx;

/* Collective hook: called on the host, with the context's stream idle, when a
 * device buffer of `count` doubles must be summed over all ranks (write_grid
 * sums, mptrac.c:13862-13872; module_mixing cell sums, mptrac.c:5289-5303).
 * A single-process run leaves it unset. */
typedef int (*mphip_allreduce_fn)(void *device_buffer, size_t count, void *user);

size_t mphip_sizeof_ctl(void);
size_t mphip_sizeof_met(void);
size_t mphip_sizeof_prep(void);   /* sizeof(mphip_prep_t), for mirrors of the structure in other languages */
/* "mptrac_amd <version> (gfx950)" -- or "(gfx950, reference rounding)" from libmptrac_hip_exact.so, the build of the
 * same sources and the same ABI whose results are the CPU reference's bits ("Two libraries") */
const char *mphip_version(void);

/* mptrac_alloc / mptrac_free: device side (acc enter/exit data,
 * mptrac.c:6336-6372, 6398-6430).  `device` is the HIP device ordinal. */
int mphip_create(mphip_ctx **ctx, int device);
void mphip_destroy(mphip_ctx *ctx);
const char *mphip_last_error(const mphip_ctx *ctx);

/* mptrac_update_device(ctl, ...), mptrac.c:8013-8018 */
int mphip_update_ctl(mphip_ctx *ctx, const mphip_ctl_t *ctl);
/* mptrac_update_device(..., clim, ...), mptrac.c:8027-8032: tropopause part of
 * clim_t (mptrac.h:3785-3800); tropo is [ntime][ld] with ld >= nlat. */
int mphip_update_clim(mphip_ctx *ctx, int ntime, int nlat, const double *tropo_time,
                      const double *tropo_lat, const double *tropo, int ld);
/* ... and one of its zonal-mean climatologies (clim_zm_t, mptrac.h:3745-3776; `which` = MPHIP_ZM_*): monthly
 * times [s since the start of the year], descending pressures [hPa], ascending latitudes [deg] and the volume
 * mixing ratios vmr[ntime][np][nlat] (the reference's index order, compact).  module_meteo needs the table of
 * every climatology quantity that is requested (hno3: also for tnat); ntime = 0 removes a table. */
/* module_oh_chem needs the OH table as well, module_h2o2_chem the H2O2 table. */
int mphip_update_clim_zm(mphip_ctx *ctx, int which, int ntime, int np, int nlat, const double *time,
                         const double *p, const double *lat, const double *vmr);
/* ... and one of its trace-gas time series (clim_ts_t, mptrac.h:3729-3743; `which` = MPHIP_TR_*): ascending times
 * [s] and volume mixing ratios; module_bound_cond sets the quantity of a series that is present to clim_ts at the
 * particle's time (constant beyond the ends of the series), ntime = 0 removes it -- the reference's
 * CLIM_*_TIMESERIES = "-". */
int mphip_update_clim_ts(mphip_ctx *ctx, int which, int ntime, const double *time, const double *vmr);
/* ... and its photolysis rates (clim_photo_t, the tables module_tracer_chem reads through clim_photo): descending
 * pressures p[np] [hPa], ascending solar zenith angles sza[nsza] [rad] and total ozone columns o3c[no3c] [DU], and per
 * trace gas (`rate` indexed by MPHIP_TR_*) the rates rate[k][np][nsza][no3c] [1/s] (the reference's index order,
 * compact); NULL: that table is absent, rate[MPHIP_TR_SF6] must be NULL.  Every axis needs two nodes or more.
 * np = 0 removes the tables.  module_tracer_chem needs the table of every present CFC / N2O quantity and the O1D
 * zonal mean (mphip_update_clim_zm). */
int mphip_update_clim_photo(mphip_ctx *ctx, int np, int nsza, int no3c, const double *p, const double *sza,
                            const double *o3c, const double *const rate[MPHIP_NTR]);
/* mptrac_update_device(..., met0, met1, ...), mptrac.c:8034-8048; slot 0 = met0,
 * slot 1 = met1. */
int mphip_update_met(mphip_ctx *ctx, int slot, const mphip_met_t *met);
/* the met0/met1 pointer swap in mptrac_get_met, mptrac.c:6488-6491.  The forward hand-over is the swap followed by
 * mphip_update_met(ctx, 1, next file); the backward hand-over of mptrac_get_met (DIRECTION -1, t < met0->time) is
 * the same swap followed by mphip_update_met(ctx, 0, earlier file): the old met0 becomes met1, and the sort and
 * interpolation axes become those of the snapshot just uploaded into slot 0. */
int mphip_swap_met(mphip_ctx *ctx);
/* The same hand-over of mptrac_get_met (read the next file into the old met0
 * buffer, swap, mptrac.c:6479-6503) with the upload taken off the stepping
 * path: mphip_prefetch_met() starts the host-to-device copies of the NEXT
 * snapshot into a third staging slot on a copy stream and returns at once
 * (an uploader thread of the library issues the copies, which keep their
 * calling thread busy for ordinary host memory; the caller's arrays must
 * stay untouched until the commit); time steps keep running on
 * met0 / met1 meanwhile.  mphip_commit_met() makes old met1 the new met0 and
 * the prefetched snapshot the new met1: the next kernel waits for the copy on
 * the device, the host does not block.  mphip_prefetch_done() = 1 once the
 * copies have finished.  mphip_prefetch_met() is the one entry point that may
 * be called from a second thread (a file reader) while another thread steps;
 * everything else, the commit included, belongs to the stepping thread (the
 * reference's interface is not re-entrant either).  Same grid dimensions as the resident snapshots
 * ("Meteo grid dimensions do not match!" otherwise, mptrac.c:6543-6546).  The pair is the FORWARD hand-over only
 * (the prefetched snapshot always becomes met1); a backward run hands over with mphip_swap_met +
 * mphip_update_met(ctx, 0, ...). */
int mphip_prefetch_met(mphip_ctx *ctx, const mphip_met_t *met);
int mphip_commit_met(mphip_ctx *ctx);
int mphip_prefetch_done(mphip_ctx *ctx);
/* drop a prefetched snapshot that will not be used (waits for its copies) */
int mphip_discard_prefetch(mphip_ctx *ctx);

/* The derived fields of the reference's meteo preprocessing, from one snapshot "as stored" (what a netCDF file of
 * MET_TYPE 0 carries): geopotential height z, total ozone column o3c, boundary-layer pressure pbl, the cloud layer pct /
 * pcb / cl, plcl / plfc / pel / cape / cin, potential vorticity pv and the tropopause pt / tt / zt / h2ot.  `in` is a host
 * view exactly as for mphip_update_met (compact or [EX][EY][EP]-strided); `what` an OR of MPHIP_PREP_* bits; the arrays
 * of `out` have the strides of `in`.  The call uploads
 * the inputs it needs into device scratch -- one pool that it shares with mphip_regrid_met and mphip_detrend_met under their
 * common lock; the pool grows to what the largest call needs, is kept between calls and freed by mphip_destroy --, runs its
 * kernels on the stream of these three calls, copies the results into the caller's arrays and returns when they are there.  It touches
 * no meteo slot, no prefetch state and no particle state and may be called from a file-reader thread while another thread
 * steps (the contract of mphip_prefetch_met); calls from several threads are serialised.  Only the outputs of the
 * requested bits are written; a refused call writes nothing.
 *   Refused: np < 2; a pressure axis that is not strictly descending; a missing input -- GEOPOT: t, h2o, ps, zs; O3C: o3,
 * ps; PBL with met_pbl 3: t, ps, ts; with met_pbl 2 additionally u, v, us, vs, zs, h2o and z, given in `in` or derived by
 * GEOPOT in the same call (the smoothed field); CLOUD: lwc, iwc, ps (rwc / swc absent = 0); CAPE: t, h2o, ps and the
 * tropopause climatology of mphip_update_clim (on a Cartesian grid also mphip_update_ctl: met_utm_ref_lat is the
 * tropopause's latitude) --; a missing output array of a requested bit; met_pbl other than 2 or 3 with PBL; smoothing
 * half-widths with sx - 1 > nx or whose tile exceeds 64 KB of LDS.  PV: t, u, v; a grid that is not longitude / latitude
 * (coord_type != 0); nx < 2 or ny < 5.  TROPO (the members met_tropo ... met_tropo_spline of `opt` are read only with this
 * bit): t, h2o and z, given in `in` or derived by GEOPOT in the same call (the smoothed field); with met_tropo 5 also pv,
 * given in `in` or derived by PV in the same call; with met_tropo 1 the tropopause climatology (and met_utm_ref_lat on a
 * Cartesian grid) as for CAPE; met_tropo outside 1 ... 5; met_tropo_spline outside 0 ... 1; np < 3 with met_tropo 2 ... 5; a
 * pressure axis with too many levels for one column's profiles in 64 KB of LDS (as for every column kernel).  All four
 * output arrays of TROPO are required.
 *
 *   DEFINITIONS.  This project's own statement of the reference's algorithms -- the reference's source was not available,
 * so no line of mptrac.c is cited --, restated independently in tests/refmetprep.py and (pv, tropopause)
 * tests/reftropo.py.  All arithmetic is in double from the
 * float inputs, products and quotients taken from left to right as written; each output value is rounded to float once.
 * exp / log / pow are the C library's.  Constants: RI = 8.3144598, MA = 28.9644, G0 = 9.80665, MO3 = 48.00, EPS =
 * 18.01528 / MA, RA = 1e3 RI / MA, CPD = 1003.5, LV = 2501000.
 *   LIN(x0,y0,x1,y1,x) = y0 + (y1-y0)/(x1-x0)*(x-x0).  P(z) = 1013.25 exp(-z/7).  THETA(p,t) = t pow(1000/p, 0.286).
 *   TVIRT(t,h) = t (1 + (1-EPS) max(h,1e-7)).  PSAT(t) = 6.112 exp(17.62 (t-273.15) / (243.12 + t - 273.15)).
 *   PW(p,h) = p max(h,1e-7) / (1 + (1-EPS) max(h,1e-7)).  SH(h) = EPS max(h,1e-7).  max(a,b) = a > b ? a : b.
 *   lapse_rate(t,h) = 1e3 G0 (a + LV r t) / (CPD a + LV LV r EPS) with a = RA (t t), r = SH(h) / (1 - SH(h)).
 *   loc(q) = the largest k in [0, np-2] with p[k] >= q, else 0.  env(f,q) = LIN(p[k],f[k],p[k+1],f[k+1],q), k = loc(q): it
 *   extrapolates beyond the ends.
 *   Geopotential (z, km).  Tv[k] = TVIRT(t[k],h2o[k]), lp[k] = log(p[k]), ZD(a,Ta,b,Tb) = RI/MA/G0 (0.5 (Ta+Tb)) (a-b).
 * k0 = loc(ps); Ts = LIN(p[k0],Tv[k0],p[k0+1],Tv[k0+1],ps); z[k0+1] = zs + ZD(log ps,Ts,lp[k0+1],Tv[k0+1]); upwards z[k] =
 * z[k-1] + ZD(lp[k-1],Tv[k-1],lp[k],Tv[k]); z[k0] = zs + ZD(log ps,Ts,lp[k0],Tv[k0]); downwards z[k] = z[k+1] +
 * ZD(lp[k+1],Tv[k+1],lp[k],Tv[k]) (the recurrences in double).  Then the float field is smoothed horizontally, per level:
 * half-widths sx, sy = met_geopot_sx, _sy; if either is negative both are automatic -- 3, 2 if |lon[1]-lon[0]| < 0.5, else 6,
 * 4 --; if either is 0: no smoothing.  For ix2 = ix-sx+1 ... ix+sx-1 (outer loop; wrapped once by +-nx, on regional grids
 * too) and iy2 = max(iy-sy+1,0) ... min(iy+sy-1,ny-1) (inner loop), over the finite values: float weight w = (1 -
 * |ix-ix2|/sx) (1 - |iy-iy2|/sy), float sums of w z and of w in that order, never contracted; the result is the quotient, or
 * NaN without a finite neighbour.
 *   Ozone column (o3c, DU).  Sum over k = 1 ... np-1 with p[k-1] <= ps of 0.5 (o3[k-1]+o3[k]) MO3 / MA (p[k-1]-p[k]) 100 /
 * G0, divided by 2.1415e-5.
 *   Cloud.  pct = pcb = NaN, cl = 0.  For k = 0 ... np-2, skipping p[k] > ps and p[k] < P(20): if any of lwc, rwc, iwc,
 * swc[k] > met_cloud_min: pct = 0.5 (p[k]+p[k+1]) and, if pcb is still NaN, pcb = 0.5 (p[k]+p[max(k-1,0)]); then (cloud or
 * not) cl += 0.5 S 100 (p[k]-p[k+1]) / G0 with S = (lwc[k]+lwc[k+1]) + (rwc[k]+rwc[k+1]) + (iwc[k]+iwc[k+1]) +
 * (swc[k]+swc[k+1]).
 *   PBL 3.  th0 = THETA(ps,ts); k runs from np-2 down to 1 and stops at the first k with p[k] >= 300 and (p[k] > ps or
 * THETA(p[k],t[k]) <= th0+2), it ends at 0 otherwise; pbl = LIN(th[k+1],p[k+1],th[k],p[k],th0+2), th[k] = THETA(p[k],t[k]).
 * Clamps: pmin = ps exp(-met_pbl_min/7); if pbl is not finite or pbl > pmin or p[k] > ps: pbl = pmin; pmax = ps
 * exp(-met_pbl_max/7); if pbl < pmax: pbl = pmax.
 *   PBL 2.  pb = ps exp(-0.05/7); k = the first level >= 1 with p[k] < pb (np-1 if there is none); h2os =
 * LIN(p[k-1],h2o[k-1],p[k],h2o[k],pb); tvs = TVIRT(THETA(pb,ts),h2os); pbl = pb, rib_old = 0; upwards from k: vh2 =
 * max((u[k]-us)^2 + (v[k]-vs)^2, 25); rib = G0 1e3 (z[k]-zs) / tvs (TVIRT(THETA(p[k],t[k]),h2o[k]) - tvs) / vh2; at the first
 * rib >= 0.25: pbl = min(LIN(rib_old,p[k-1],rib,p[k],0.25), pb) and stop (min(a,b) = a < b ? a : b), else rib_old = rib.
 * Then the two clamps of PBL 3 (every p[k] visited lies above the surface: that term drops out).
 *   CAPE.  pfac = 1.01439, dz0 = RI/MA/G0 log(pfac).  pbot = min(ps,p[0]); th, h = mean THETA(p[k],t[k]) and mean h2o[k]
 * over the levels with pbot >= p[k] >= pbot-50 (stop at the first level below pbot-50 once one was taken); plcl = plfc = pel =
 * cape = cin = NaN; if h <= 0 or no level was taken: done.  Lifted condensation level: ptop = P(20), pbot = ps; do { plcl =
 * 0.5 (pbot+ptop); t = th / pow(1000/plcl, 0.286); if (100 PW(plcl,h) / PSAT(t) > 100) ptop = plcl; else pbot = plcl; }
 * while (pbot - ptop > 0.1).  cape = cin = 0, p = ps; do { dz = dz0 TVIRT(t,h); p /= pfac; t = th / pow(1000/p, 0.286); Te =
 * env(t,p), he = env(h2o,p); d = 1e3 G0 (TVIRT(t,h) - TVIRT(Te,he)) / TVIRT(Te,he) dz; if (d < 0) cin += |d|; } while (p >
 * plcl).  d = 0, p = plcl, t = th / pow(1000/p, 0.286), ptop = 0.75 clim_tropo(time, lat) (the climatological tropopause of
 * mphip_update_clim at the column's latitude, met_utm_ref_lat on a Cartesian grid); do { dz = dz0 TVIRT(t,h); p /= pfac; t -=
 * lapse_rate(t,h) dz; e = PSAT(t); h = e / (p - (1-EPS) e); Te, he as above; d_old = d; d = the same expression; if (d > 0) {
 * cape += d; if plfc is NaN: plfc = p; } else if (d_old > 0) pel = p; if (d < 0 and plfc is NaN) cin += |d|; } while (p >
 * ptop).  If plfc is NaN: cin = NaN.  (An infinite ps is taken as NaN, here and in the geopotential, so that every loop ends: p
 * shrinks by pfac per pass and a NaN makes each condition false.)
 *   Further helpers (each a function: its value is formed before it enters the expression around it; cos and sin are the
 * C library's).  RE = 6367.421.  RAD(x) = x (M_PI / 180.0).  DEG2DX(d,lat) = RE RAD(d) cos(RAD(lat)).  DEG2DY(d) = RE
 * RAD(d).  Z(p) = 7 log(1013.25 / p).  LAPSE(p1,t1,p2,t2) = 1e3 G0 / RA (t2 - t1) / (t2 + t1) (p2 + p1) / (p2 - p1).
 *   Potential vorticity (pv, PVU).  pows[k] = pow(1000/p[k], 0.286).  Per column (ix, iy): ix0 = max(ix-1,0), ix1 =
 * min(ix+1,nx-1) (clamped, not wrapped), iy0, iy1 likewise; latr = 0.5 (lat[iy1] + lat[iy0]); dx = 1000
 * DEG2DX(lon[ix1]-lon[ix0], latr); dy = 1000 DEG2DY(lat[iy1]-lat[iy0]); c0 = cos(RAD(lat[iy0])), c1 = cos(RAD(lat[iy1])),
 * cr = cos(RAD(latr)); vort = 2 * 2 * M_PI / 86400. * sin(RAD(lat[iy])).  Per level k: dtdx = (t[ix1][iy][k] - t[ix0][iy][k])
 * pows[k] / dx; dvdx = (v[ix1][iy][k] - v[ix0][iy][k]) / dx; dtdy = (t[ix][iy1][k] - t[ix][iy0][k]) pows[k] / dy; dudy =
 * (u[ix][iy1][k] c1 - u[ix][iy0][k] c0) / dy; k0 = max(k-1,0), k1 = min(k+1,np-1), dp0 = 100 (p[k]-p[k0]), dp1 = 100
 * (p[k1]-p[k]); for a column profile a, in the interior (k != k0 and k != k1) D(a) = (dp0 dp0 a[k1] - dp1 dp1 a[k0] + (dp1
 * dp1 - dp0 dp0) a[k]) / (dp0 dp1 (dp0+dp1)), at the two end levels D(a) = (a[k1] - a[k0]) / (dp0 + dp1); dtdp = D(t pows)
 * (a[k] = t[k] pows[k]), dudp = D(u), dvdp = D(v); pv = 1e6 G0 (-dtdp (dvdx - dudy / cr + vort) + dvdp dtdx - dudp dtdy).
 * After all columns, for every ix and k and by index, for either latitude order: rows 0 and 1 take row 2's value, rows ny-1
 * and ny-2 row ny-3's.
 *   Tropopause (pt hPa, tt K, zt km, h2ot ppv).  zc[k] = Z(p[k]) (ascending); z2[i] = 4.5 + 0.1 i, p2[i] = P(z2[i]), i = 0
 * ... 200.  spline(y)[i] for a column profile y on zc: y[0] if z2[i] <= zc[0]; y[np-1] if z2[i] >= zc[np-1]; otherwise, with
 * k the largest index with zc[k] <= z2[i] and k <= np-2: met_tropo_spline 0: LIN(zc[k],y[k],zc[k+1],y[k+1],z2[i]);
 * met_tropo_spline 1, the natural cubic spline: h[k] = zc[k+1]-zc[k]; c[0] = c[np-1] = 0; for i = 0 ... np-3: d[i] = 2
 * (h[i]+h[i+1]), o[i] = h[i+1], g[i] = 3 ((y[i+2]-y[i+1]) / h[i+1] - (y[i+1]-y[i]) / h[i]); forward, for i = 1 ... np-3: w =
 * o[i-1] / d[i-1]; d[i] -= w o[i-1]; g[i] -= w g[i-1]; back: c[np-2] = g[np-3] / d[np-3], then c[i+1] = (g[i] - o[i] c[i+2]) /
 * d[i] for i = np-4 down to 0; value: h = h[k], b = (y[k+1]-y[k]) / h - h (c[k+1] + 2 c[k]) / 3, e = (c[k+1]-c[k]) / (3 h),
 * dx = z2[i]-zc[k], result y[k] + dx (b + dx (c[k] + dx e)).  A NaN among the fine values a mode looks at makes pt NaN.
 *   met_tropo 1: pt = clim_tropo(time, lat[iy]) (met_utm_ref_lat on a Cartesian grid).  2 (cold point): t2 = spline(t) on i
 * = 0 ... 170; iz = the first index of the minimum; pt = p2[iz] if 0 < iz < 170, else NaN.  3 (WMO): t2 on i = 0 ... 200;
 * B(iz): LAPSE(p2[iz],t2[iz],p2[j],t2[j]) <= 2.0 for every j = iz+1 ... iz+20; iz1 = the first iz in 0 ... 170 with B; pt =
 * p2[iz1] if it exists and 0 < iz1 < 170, else NaN.  4 (WMO, second tropopause): iz1 as for 3, NaN if there is none; A(iz):
 * LAPSE(...) >= 3.0 for every j = iz+1 ... iz+10; iza = the first iz in iz1 ... 170 with A; iz2 = the first iz in iza ... 170
 * with B; pt = p2[iz2] if it exists and 0 < iz2 < 170, else NaN.  5 (dynamical): pv2 = spline(pv), th2 =
 * spline(THETA(p[k],t[k])) on 0 ... 170; iz = the first index with fabs(pv2[iz]) >= met_tropo_pv or th2[iz] >=
 * met_tropo_theta; pt = p2[iz] if it exists and 0 < iz < 170, else NaN.  Then tt = env(t,pt), zt = env(z,pt), h2ot =
 * env(h2o,pt); all three NaN when pt is NaN.
 *   Values outside the physical range are not refused: the arithmetic above decides, by IEEE rules and with the C library's
 * results (log 0 = -inf, log of a negative number NaN, 1000/0 = inf, pow(x, 0.286) NaN for x < 0 and 0 for x = -0), and
 * every comparison with a NaN is false.  So max(h, 1e-7) takes a NaN h for 1e-7 -- TVIRT, PW and SH treat a NaN water
 * vapour as the dry floor -- and min(ps, p[0]) a NaN ps for p[0]; loc(NaN) = 0, and loc(q) = np-2 for every q <= p[np-2], q
 * <= 0 included.  The geopotential and CAPE take an infinite ps as NaN; the ozone column, the cloud layer and the boundary
 * layer take it as it is.  The outcomes (tests/metprep_cases.py, `nonfinite`):
 *   ps NaN: z NaN on every level; o3c = 0; no level is skipped by the cloud search; pbl NaN; the parcel is that of p[0],
 * every loop of CAPE ends in its first pass: cape = 0, plcl = plfc = pel = cin = NaN.  ps = +inf: z and CAPE as for NaN;
 * o3c and the cloud layer are those of the whole column; pbl = +inf.  ps = -inf: z and CAPE as for NaN; o3c = 0, pct = pcb =
 * NaN, cl = 0; pbl = -inf.  ps = 0: z = -inf on every level (the smoothing skips it like a NaN: it sums finite values
 * only); o3c = 0, pct = pcb = NaN, cl = 0; no level lies at or below the surface, so no parcel: the five CAPE outputs are
 * NaN; pbl = 0.  ps < 0: as for 0, but z NaN (log ps) and pbl = ps exp(-met_pbl_max/7) (pmin < pmax there, and the second
 * clamp is the last).  A NaN in t[k] makes z NaN on the levels from k away from the surface (on all levels if the surface's
 * LIN reads it); an infinite h2o makes z NaN on every level; a NaN zs makes z NaN on every level; a NaN ts makes PBL 3's pbl
 * pmin (it is not finite) and keeps PBL 2's criterion false, which is pmin as well.
 *   Out of scope: MET_PBL 1.  (Down-sampling and model-to-pressure-level regridding: mphip_regrid_met; detrending:
 * mphip_detrend_met.) */
enum { MPHIP_PREP_GEOPOT = 1, MPHIP_PREP_O3C = 2, MPHIP_PREP_PBL = 4, MPHIP_PREP_CLOUD = 8, MPHIP_PREP_CAPE = 16,
       MPHIP_PREP_PV = 32, MPHIP_PREP_TROPO = 64 };
typedef struct {
  int met_pbl;                        /* 2: bulk Richardson number, 3: potential temperature */
  double met_pbl_min, met_pbl_max;    /* km; reference defaults 0.1, 5.0 */
  int met_geopot_sx, met_geopot_sy;   /* smoothing half-widths; < 0: automatic, 0: none */
  double met_cloud_min;
  /* read only with MPHIP_PREP_TROPO (appended: the members above keep their offsets) */
  int met_tropo;                      /* 1 climatology, 2 cold point, 3 WMO, 4 second WMO, 5 dynamical; reference default 3 */
  double met_tropo_pv;                /* PVU; reference default 3.5 */
  double met_tropo_theta;             /* K; reference default 380 */
  int met_tropo_spline;               /* 1: cubic, 0: linear; reference default 1 */
} mphip_prep_t;
typedef struct {
  float *f3[MPHIP_N3D];
  float *f2[MPHIP_N2D];
} mphip_met_out_t;   /* same strides as `in` */
int mphip_derive_met(mphip_ctx *ctx, const mphip_met_t *in, unsigned what, const mphip_prep_t *opt,
                     const mphip_met_out_t *out);

/* The two grid-changing steps of the reference's meteo preprocessing, from one snapshot "as stored": model levels to
 * pressure levels (MPHIP_REGRID_ML2PL, the reference's read_met_ml2pl) and smoothing with down-sampling
 * (MPHIP_REGRID_SAMPLE, read_met_sample).  `in` is a host view as for mphip_derive_met; the shape changes, so `out` names
 * its own strides (as mphip_met_t does: sy >= np2, sx a multiple of sy and >= ny2 sy, sx2 >= ny2) and the output axes.
 * mphip_regrid_shape gives the output extents without a context, so that a caller can allocate; it returns non-zero
 * where mphip_regrid_met would refuse the grid or the options.  The call keeps the contract of mphip_derive_met: the same
 * stream and lock (calls are serialised with mphip_derive_met), the same scratch pool (grow-only, freed by
 * mphip_destroy), no meteo slot, no prefetch state and no particle touched, callable from a file-reader thread, and a
 * refused call writes nothing.  Every input is uploaded before any output is written, so `out` may alias `in` (the host
 * layer regrids its met_t in place).  Fields that are NULL in `in` or NULL in `out` are skipped, axes that are NULL in `out`
 * likewise.  With both bits ML2PL runs first and SAMPLE works on its result on the device.  The model-level slots
 * (MPHIP_PL, UL, VL, WL, ZETAL, ZETA_DOTL) are never written.
 *
 *   DEFINITIONS.  This project's own statement, as for mphip_derive_met (the reference's source was not available),
 * restated independently in tests/refregrid.py.  Arithmetic in double from the float inputs unless "float" is written,
 * products and quotients from left to right, each output value rounded to float once; LIN as above.
 *   ML2PL.  Input: n = in->npl model levels, in->np == in->npl; in->f3[MPHIP_PL] the pressure [hPa] with the strides sx_ml,
 * sy_ml; the fields are the non-NULL slots MPHIP_T, U, V, W, H2O, O3, LWC, RWC, IWC, SWC, CC with the strides sx, sy and n
 * levels; in->p is not read.  Per column, pl[0 ... n-1], and per target level j, q = met_p[j]:  clamp -- if pl[0] > pl[1]:
 * { if (q > pl[0]) q = pl[0]; else if (q < pl[n-1]) q = pl[n-1]; } else { if (q < pl[0]) q = pl[0]; else if (q > pl[n-1]) q =
 * pl[n-1]; } --; k = locate_irr(pl, n, q): ilo = 0, ihi = n-1, i = (ihi+ilo)>>1; if (pl[i] < pl[i+1]) while (ihi > ilo+1) { i
 * = (ihi+ilo)>>1; if (pl[i] > q) ihi = i; else ilo = i; } else while (ihi > ilo+1) { i = (ihi+ilo)>>1; if (pl[i] <= q) ihi =
 * i; else ilo = i; }; k = ilo (on a strictly descending column the largest k <= n-2 with pl[k] > q, else 0); out[j] =
 * LIN(pl[k], f[k], pl[k+1], f[k+1], q).  Nothing is refused for its values: equal neighbouring pressures, NaN and
 * non-monotone columns give what IEEE arithmetic and the bisection as written give.  The 2-D fields, lon and lat pass
 * through; out->p = met_p; np2 = met_np.
 *   Refused: npl < 2 or np != npl; a missing MPHIP_PL; met_np < 2; a met_p that is not finite, positive and strictly
 * descending; a level count whose staged columns do not fit 64 KB of LDS (8 met_np + 4 (npl | 1) bytes for one column).
 *   SAMPLE.  Input: a pressure-level snapshot (nx, ny, np, axes lon, lat, p) or the result of ML2PL.  nx2 = (nx + met_dx -
 * 1) / met_dx, ny2 and np2 likewise; output index i is input index i met_dx; lon, lat and p are sampled the same way.
 * With sx, sy, sp = met_sx, met_sy, met_sp: for every kept point (ix, iy, ip) of every non-NULL 3-D pressure-level field
 * (the eleven above, MPHIP_Z and MPHIP_PV): if sx = sy = sp = 1 the value is copied.  Otherwise float sums a = 0, ws = 0;
 * for ix2 = ix-sx+1 ... ix+sx-1 (outer loop; ix3 = ix2 wrapped once by +-nx, on regional grids too), iy2 = max(iy-sy+1,0)
 * ... min(iy+sy-1,ny-1) (middle loop), ip2 = max(ip-sp+1,0) ... min(ip+sp-1,np-1) (inner loop): float w = (1 -
 * |ix-ix2|/sx) (1 - |iy-iy2|/sy) (1 - |ip-ip2|/sp), each factor formed in float (a float quotient, a float difference) and
 * multiplied from left to right; a += w f[ix3][iy2][ip2] (the product rounded before the sum, never contracted); ws += w.
 * The value is a / ws in float.  Every value enters: a NaN spreads (unlike the geopotential's smoothing).  Every non-NULL
 * 2-D field gets the same with the two horizontal factors only (copied if sx = sy = 1).  Only the kept points are
 * computed.  With all six options 1 the output is the input, bit for bit.
 *   Refused: an option < 1; met_sx - 1 > nx; nx2 < 2, ny2 < 2 or np2 < 2; a tile with halo beyond 64 KB of LDS -- hx hy hk
 * floats with hx = 7 min(met_dx, 2 sx - 1) + 2 sx - 1, hy = 7 min(met_dy, 2 sy - 1) + 2 sy - 1, hk = 15 min(met_dp, 2 sp -
 * 1) + 2 sp - 1.
 *   Both: refused as either; nx < 2, ny < 2, strides that do not hold the extents, a missing axis (lon, lat; p for SAMPLE
 * alone), `what` other than an OR of the two bits. */
enum { MPHIP_REGRID_ML2PL = 1, MPHIP_REGRID_SAMPLE = 2 };
typedef struct {
  int met_np; const double *met_p;      /* ML2PL: target pressure levels [hPa] */
  int met_dx, met_dy, met_dp;           /* SAMPLE: keep every dx-th longitude, dy-th latitude, dp-th level */
  int met_sx, met_sy, met_sp;           /* SAMPLE: smoothing half-widths (1 = none) */
} mphip_regrid_t;
typedef struct {                        /* the caller's arrays and their strides: the shape changes */
  long long sx, sy, sx2;
  double *lon, *lat, *p;                /* the output axes (nx2, ny2, np2 values) */
  float *f3[MPHIP_N3D]; float *f2[MPHIP_N2D];
} mphip_regrid_out_t;
size_t mphip_sizeof_regrid(void);       /* sizeof(mphip_regrid_t), for mirrors of the structure in other languages */
int mphip_regrid_shape(const mphip_met_t *in, unsigned what, const mphip_regrid_t *opt, int *nx2, int *ny2, int *np2);
int mphip_regrid_met(mphip_ctx *ctx, const mphip_met_t *in, unsigned what, const mphip_regrid_t *opt,
                     const mphip_regrid_out_t *out);

/* Detrending (the reference's read_met_detrend): a Gaussian-weighted horizontal mean, the background, is subtracted from
 * t, u, v and w of a pressure-level snapshot on a longitude / latitude grid.  The call keeps the contract of
 * mphip_derive_met / mphip_regrid_met: the same stream and lock, the same scratch pool (grow-only, freed by
 * mphip_destroy), no meteo slot, no prefetch state and no particle touched, callable from a file-reader thread while
 * another thread steps; a refused call writes nothing and its message starts with "mphip_detrend_met: ".  Every input
 * is uploaded and the weights are built before any output is copied back, so `out` may alias `in`.  The shape does not
 * change: `out` names the strides of its arrays (sy >= np, sx a multiple of sy and >= ny sy), only out->f3[MPHIP_T],
 * [MPHIP_U], [MPHIP_V] and [MPHIP_W] are written, a field that is NULL in `in` or in `out` is skipped, and the axes and
 * every other slot of `out` are ignored.
 *
 *   DEFINITION.  This project's own statement, as for mphip_derive_met (the reference's source was not available),
 * restated independently in tests/refdetrend.py.  RE, RAD and M_PI as above; cos, sin and exp are the C library's;
 * products, quotients and sums from left to right as written.  DX2DEG(dx,lat) = (lat < -89.999 || lat > 89.999) ? 0 : dx
 * 180. / (M_PI RE cos(RAD(lat))).  DY2DEG(dy) = dy 180. / (M_PI RE).  geo2cart(z,lon,lat) = ((RE+z) cos(RAD(lat))
 * cos(RAD(lon)), (RE+z) cos(RAD(lat)) sin(RAD(lon)), (RE+z) sin(RAD(lat))).  DIST2(a,b) = (a0-b0)(a0-b0) + (a1-b1)(a1-b1)
 * + (a2-b2)(a2-b2).
 *   In double: sigma = met_detrend / 2.355; tssq = 2. sigma sigma; dlon = |lon[1]-lon[0]|, dlat = |lat[1]-lat[0]|; sy =
 * (int) (3. DY2DEG(sigma) / dlat) limited to [1, ny/2]; per row iy: sx(iy) = (int) (3. DX2DEG(sigma, lat[iy]) / dlon)
 * limited to [1, nx/2] (integer halves; a quotient that is not below the upper limit gives the upper limit, so nothing
 * depends on converting a value beyond the int range).  Next to the poles DX2DEG is 0 and sx = 1.
 *   Weights: w(iy, iy2, d) = (float) exp(-D2 / tssq) with D2 = DIST2(geo2cart(0, 0, lat[iy]), geo2cart(0, d dlon,
 * lat[iy2])) and d = |ix - ix2|: the weight depends on the row pair and the longitude offset only.  The reference
 * evaluates geo2cart at the actual longitudes lon[ix], lon[ix2]; on a regular axis the two agree in exact arithmetic (the
 * distance of two points depends on their longitude difference only), not always in the last bit.  This form was chosen
 * because it makes the weights one table per call -- sum over iy of (rows in range) (sx(iy) + 1) floats, built on the
 * host with the C library as the tropopause's tables are, so both libraries and the restatement use the same bits --,
 * leaves no exp inside the stencil, and makes the weight uniform across a wave (one row per workgroup: a scalar
 * operand).
 *   Accumulation, for every point (ix, iy, ip) of every present field f: float b = 0, ws = 0; for ix2 = ix-sx ... ix+sx
 * (outer loop; ix3 = ix2 wrapped once by +-nx, on regional grids too and with a periodic extra column present), iy2 =
 * max(iy-sy,0) ... min(iy+sy,ny-1) (inner loop): ws += w; b += w f[ix3][iy2][ip] (the product rounded to float before
 * the sum, never contracted).  out = f[ix][iy][ip] - b / ws, float throughout.  Every value enters: a NaN or an infinity
 * spreads as IEEE arithmetic gives it.  Both libraries return these bits (the division is IEEE in both).
 *   Refused: a NULL argument or axis (lon, lat, p); nx < 2, ny < 2, np < 2; nx ny >= 2^24 or nx ny np >= 2^31; strides
 * that do not hold the extents; coord_type != 0; a met_detrend that is not finite or <= 0; dlon or dlat zero or not
 * finite; none of the four fields present on both sides.  Nothing is refused for a large half-width. */
typedef struct {
  double met_detrend;                   /* full width at half maximum of the background's Gaussian [km] */
} mphip_detrend_t;
size_t mphip_sizeof_detrend(void);      /* sizeof(mphip_detrend_t), for mirrors of the structure in other languages */
int mphip_detrend_met(mphip_ctx *ctx, const mphip_met_t *in, const mphip_detrend_t *opt, const mphip_regrid_out_t *out);

/* Ingest: what lies between the values a netCDF file (MET_TYPE 0) stores and a met_t -- decoding of packed shorts, the
 * fill / missing-value mask, the unit scale, the re-ordering from the file's [level][y][x] to met_t's [x][y][level], the
 * surface pressure from its logarithm, the extrapolation below the lowest valid level, the pole rows of the winds and
 * the periodic longitude column.  The call keeps the contract of mphip_derive_met / mphip_regrid_met /
 * mphip_detrend_met: the same stream and lock, the same scratch pool (grow-only, freed by mphip_destroy), no meteo slot,
 * no prefetch state and no particle touched, callable from a file-reader thread while another thread steps; a refused
 * call writes nothing and its message starts with "mphip_ingest_met: ".  Every input is uploaded before any output is
 * copied back, so met-order outputs may alias met-order inputs (the host layer works on its met_t in place).
 *   `what` is an OR of MPHIP_INGEST_* bits; the stages always run in the order DECODE, EXTRAPOLATE, POLAR, PERIODIC.
 *   Input.  The axes (lon, lat, p), the extents nx, ny, np (npl: the levels of the model-level slots MPHIP_PL, UL, VL,
 * ZETAL, ZETA_DOTL, WL) and coord_type come from `in`.  With DECODE a slot whose descriptor in `raw` has a type other than
 * 0 is read from that descriptor: `data` in file order, [nlev][ny][nx] or [ny][nx], host-endian.  Every other slot, and
 * every slot without DECODE (`raw` may be NULL then), is read from in->f3 / in->f2 in met order, strided as for
 * mphip_detrend_met (sx_ml, sy_ml for the model-level slots).  The second form is what a model-level file needs, where
 * mphip_regrid_met(ML2PL) runs between DECODE and the other stages.
 *   Output.  `out` names its arrays, their strides (sy >= the levels of every field named, sx a multiple of sy and >= ny
 * sy, sx2 >= ny; the model-level slots use sx, sy as well) and the axes: lon gets nx2 values, lat ny, p np; an axis that is
 * NULL is skipped.  A slot that is absent on the input side or NULL in `out` is skipped.  Every slot present on both
 * sides is written, with nx2 columns, whichever stages run.
 *
 *   DEFINITIONS, transcribed from the host loops of read_met_nc in mptrac_amd/host/mptrac.c (nc_field, the lnsp
 * conversion, the extrapolation loop behind "Pressure levels must be descending", met_polar_winds /
 * pole_row_from_neighbour, met_periodic), which tests/test_ingest_cpu.py pins to the restatement tests/refingest.py.
 * Every operation is the IEEE operation on the named type, rounded once and never contracted, in BOTH libraries; NAN is
 * the quiet NaN 0x7fc00000; exp, cos and sin are the C library's (mphip_libm.h on the device).
 *   DECODE, MPHIP_RAW_SHORT (shorts are always packed; an unpacked short variable stays the reader's float conversion):
 * float v = (float) raw * scale_factor + add_offset, a float product and then a float sum; keep = (fill_s == 0 || raw !=
 * fill_s) && (miss_s == 0 || raw != miss_s) && fabsf(v) < 1e14f; out = keep ? scl * v : NAN.  fill and miss are already
 * converted to the stored type, 0 meaning "none", exactly as nc_field forms fillval / missval.
 *   DECODE, MPHIP_RAW_FLOAT: the same with v the stored value and float comparisons against fill_f, miss_f.  A NaN or
 * infinite stored value therefore gives NAN, and a NaN fill masks nothing.
 *   DECODE, lnsp (MPHIP_PS only): after the above (the reader passes scl = 1), ps = (float) (exp((double) out) / 100.).
 *   DECODE, placement: the value of file index (k, j, i) lands at [i][j][k].
 *   EXTRAPOLATE.  Per column, low = the largest level index at which t, u, v or w is not finite, or -1; a field of the
 * four that is absent counts as finite.  Every present level field of t, u, v, w, h2o, o3, lwc, rwc, iwc, swc, cc gets f[k]
 * = f[low + 1] for k <= low; bits are copied, so NaN payloads survive.  If low == np - 1 the column is filled with 0.f.
 * (This is this project's definition.  The host loop reads element np of the fixed-extent array [EP] there -- zero in a
 * fresh met_t, whatever an earlier and larger file left there otherwise -- or 0.f when np == EP.  The host loop is left
 * as it is.)
 *   POLAR.  Runs only if coord_type == 0, |lat[0]| >= 89.999 and |lat[ny-1]| >= 89.999, and u and v are both present.  Per
 * pole row the tables c[ix] = cos(turn lon[ix] (M_PI / 180.0)), s[ix] = sin(turn lon[ix] (M_PI / 180.0)) with turn =
 * lat[pole] < 0 ? -1 : 1 are built by the host inside the call.  Per pole and level the double sums run over ix = 0 ...
 * nx-1 in that order: mx += (u c - v s) / nx, my += (u s + v c) / nx with u, v of the neighbour row -- two products, one
 * difference or sum and one true division by (double) nx each --, then u = (float) (mx c + my s), v = (float) (my c - mx
 * s) on the pole row.  The rows are done in the order {0 from 1}, {ny-1 from ny-2}: with ny == 2 the second reads what the
 * first wrote.  nx is the extent before the periodic column is added.
 *   PERIODIC.  Runs only if coord_type == 0 and fabs(lon[nx-1] - lon[0] + lon[1] - lon[0] - 360) < 0.01.  nx2 = nx + 1,
 * lon[nx] = lon[nx-1] + lon[1] - lon[0], and column nx of every present field, the model-level slots included, is a copy
 * of column 0.  Otherwise nx2 = nx.  mphip_ingest_shape answers nx2 without a context (non-zero where the call would
 * refuse the grid or `what`).  A caller with arrays of a fixed extent checks nx2 against it before the call.
 *   Refused: a NULL argument (raw with DECODE) or a missing axis (lon, lat, p); nx < 2, ny < 2, np < 2; nx2 ny >= 2^24 or
 * nx2 ny nlev >= 2^31; input strides that do not hold a met-order field that is read; output strides that do not hold ny
 * and the levels; a descriptor with a type other than 0, MPHIP_RAW_FLOAT, MPHIP_RAW_SHORT; a descriptor with NULL data
 * for a field that `out` names; DECODE with a field given both raw and in in->f3 / in->f2; a `what` outside the four
 * bits, or 0; lnsp on a slot other than MPHIP_PS; a model-level slot with npl < 1; no field present on both sides. */
enum { MPHIP_INGEST_DECODE = 1, MPHIP_INGEST_EXTRAPOLATE = 2, MPHIP_INGEST_POLAR = 4, MPHIP_INGEST_PERIODIC = 8 };
enum { MPHIP_RAW_FLOAT = 1, MPHIP_RAW_SHORT = 2 };
typedef struct {
  const void *data;                     /* float or short values in file order; NULL with type 0 */
  int type;                             /* 0: the slot is not given raw */
  int lnsp;                             /* MPHIP_PS only: the values are the logarithm of the surface pressure in Pa */
  float scale_factor, add_offset;       /* MPHIP_RAW_SHORT */
  float fill_f, miss_f;                 /* MPHIP_RAW_FLOAT: _FillValue, missing_value as floats (0: none) */
  short fill_s, miss_s;                 /* MPHIP_RAW_SHORT: ... as shorts (0: none) */
  float scl;                            /* the unit scale */
} mphip_raw_t;
typedef struct {
  mphip_raw_t f3[MPHIP_N3D];
  mphip_raw_t f2[MPHIP_N2D];
} mphip_ingest_raw_t;
size_t mphip_sizeof_ingest_raw(void);   /* sizeof(mphip_ingest_raw_t), for mirrors of the structure in other languages */
int mphip_ingest_shape(const mphip_met_t *in, unsigned what, int *nx2);
int mphip_ingest_met(mphip_ctx *ctx, const mphip_met_t *in, const mphip_ingest_raw_t *raw, unsigned what,
                     const mphip_regrid_out_t *out);

/* 16-bit packed level fields (the reference's MET_TYPE 2 files): every level field as unsigned 16-bit codes with one scale
 * and one offset per level -- half the bytes on disk and over PCIe.  The codes travel to the device as they are and become
 * floats there (2 bytes read and 4 written per value, once per snapshot); no arithmetic on meteo values on the host.
 *
 *   DEFINITION.  This project's own statement (the reference's source was not available), restated independently in
 * tests/refpack.py.  A level field is nx ny columns of nlev values, level fastest: the compact [ix][iy][ip] order of a
 * MET_TYPE 1 file.  Every operation below is the IEEE operation on the named type, rounded once, never fused with its
 * neighbour; both libraries return these bits.
 *   Decoding, code q (0 ... 65535, every one of them, also 65534 and 65535, which the encoder never writes) at level ip:
 * v = (float) ((double) q * scl[ip] + off[ip]) -- the product rounded to double, the sum rounded to double, then one
 * rounding to float --, then the limits of the reader, fminf(fmaxf(v, lo), hi) as the C library evaluates them: v < lo or
 * v a NaN gives lo, v > hi gives hi, and a zero that compares equal to a limit keeps its own sign.  scl / off that are
 * not finite are not refused: they decode to what the arithmetic gives.
 *   Encoding, per level: min and max over all columns, compared as doubles; off = min + 0. (a minimum that is a zero of
 * either sign is stored as +0.: the result does not depend on the order in which the values were compared); scl = (max !=
 * min) ? (max - min) / 65533. : 1.; q = (unsigned short) (((double) x - off) / scl + .5), a true division, truncated.  The
 * largest code written is 65533.  A level that holds a value that is not finite has no code: the call is refused.
 *   File (MET_TYPE 2, extension pck): [2] [104] time nx ny np lon[] lat[] p[]; the 24 surface fields as raw floats as in a
 * MET_TYPE 1 file; the 13 level fields in the same order, each scl[np] doubles, off[np] doubles, nx ny np unsigned shorts;
 * [999].
 *
 * mphip_met_packed_t describes a snapshot some of whose level fields are codes: `base` carries the axes, extents,
 * strides, the surface fields and the level fields that stay float; q3[f] the compact codes [nx][ny][nlev] of field f
 * (nlev = np, or npl for the model-level fields), scl[f] / off[f] their nlev scales and offsets, lo[f] / hi[f] the limits
 * applied after decoding.  A field is given in base.f3 or in q3, never both. */
typedef struct {
  mphip_met_t base;
  const unsigned short *q3[MPHIP_N3D];
  const double *scl[MPHIP_N3D], *off[MPHIP_N3D];
  float lo[MPHIP_N3D], hi[MPHIP_N3D];
} mphip_met_packed_t;
size_t mphip_sizeof_met_packed(void);   /* sizeof(mphip_met_packed_t), for mirrors of the structure in other languages */
/* mphip_update_met / mphip_prefetch_met for such a snapshot, the same in every respect (checks and messages, axes, "Meteo
 * grid dimensions do not match!", what may be called from which thread): a packed field is uploaded as codes into a
 * grow-only code buffer -- one per stream, sized for the largest field, reused in stream order, freed with the slot arrays
 * on a new grid and by mphip_destroy -- and decoded behind its copy into the staging array a float upload fills; nothing
 * behind the staging arrays differs.  Refused with a message, nothing written: a field given both ways, codes without scl
 * or off, lo > hi (or a limit that is a NaN). */
int mphip_update_met_packed(mphip_ctx *ctx, int slot, const mphip_met_packed_t *met);
int mphip_prefetch_met_packed(mphip_ctx *ctx, const mphip_met_packed_t *met);
/* Decoding and encoding between host arrays, members of the family of mphip_derive_met (the same stream, lock and scratch
 * pool; no meteo slot, no prefetch state and no particle touched; callable from a file-reader thread while another thread
 * steps; a refused call writes nothing; every input is uploaded before an output is copied back).  The float arrays may be
 * strided as for mphip_detrend_met (sy >= nlev, sx a multiple of sy and >= ny sy; base.sx_ml / sy_ml for the model-level
 * fields), the codes are compact.
 *   mphip_unpack_met writes out->f3[f] for every field that `in` gives as codes and `out` names (base.f3 of `in` and the
 * surface fields are ignored).  mphip_pack_met encodes in->f3[f] into the arrays out->q3[f], out->scl[f], out->off[f]
 * point to, for every field present in both (a NULL q3[f] skips the field; out->base.f3, lo and hi are ignored); a value
 * that is not finite refuses the call with the field's name and the level.  mphip_pack_met takes up to 16383 levels: a
 * column of a field is staged in 64 KB of LDS at the pitch nlev | 1 floats, and a field with more levels is refused ("too
 * many levels for one column in 64 KB of LDS") before anything is written; mphip_unpack_met and the two uploads have no
 * such limit (their scales and offsets are read from LDS up to 4096 levels and from global memory above).  Messages start
 * with the call's name. */
int mphip_unpack_met(mphip_ctx *ctx, const mphip_met_packed_t *in, const mphip_met_t *out);
int mphip_pack_met(mphip_ctx *ctx, const mphip_met_t *in, const mphip_met_packed_t *out);

/* intpol_met_time_3d / intpol_met_time_2d (mptrac.c:3112-3170) for n points of the caller: "what is field X at (t, p, lon,
 * lat)?", answered from the resident meteo pair on the device.  time has ntime entries, ntime = 1 (one time for all
 * points) or n; p, lon, lat have n; field[k] is MPHIP_U ... for a pressure-level field or MPHIP_INTPOL_2D | MPHIP_PS ...
 * for a surface field; out is [nfield][n] doubles in host memory.  p may be NULL when only surface fields are asked for.
 *   The snapshots are the resident pair as the next time step would see it: the current slots after any mphip_swap_met, a
 * packed upload as decoded, and after mphip_commit_met the new pair; a prefetch in flight is not visible.  The call runs on
 * the context's stream and belongs to the stepping thread.  It touches no particle, no packed record and no pending
 * deferred module_meteo launch.  The points travel through two grow-only buffers of the context in chunks of the option
 * "intpol_chunk" points, so device memory does not grow with n.  n = 0 succeeds and writes nothing.  Between
 * mphip_profile_begin and mphip_profile_end every kernel launch of the call is one event pair (a phase of its own when
 * only this call is made in between).
 *
 *   DEFINITION.  Per point, one index and weight set from the CURRENT met0's axes, shared by all fields (INTPOL_TIME_ALL,
 * mptrac.h:1278-1318): the horizontal check by coord_type -- 0: lon2 = FMOD(lon, 360), plus 360 if below lon[0], else minus
 * 360 if above lon[nx-1]; otherwise lon clamped to the axis; lat clamped to the axis --, ip = locate_irr(p), ix =
 * locate_reg(lon2), iy = locate_irr(lat2), wp = (p[ip+1] - p) / (p[ip+1] - p[ip]) and wx, wy likewise: true divisions.
 * Pressure-level field, on met0 and on met1 with met0's indices: vertical blend wp (a[ip] - a[ip+1]) + a[ip+1] at the four
 * columns (the difference of the two floats is a float difference, as in the reference; everything else is double), then latitude, then longitude, then in time with wt = (time1 - t) / (time1 - time0): wt (v0 - v1) + v1.  Surface
 * field: the same two horizontal blends if all four corners are finite, else the nearest corner (wx < 0.5 ? ix+1 : ix, wy <
 * 0.5 ? iy+1 : iy); in time the blend if both values are finite, else the nearer snapshot (wt < 0.5 ? v1 : v0).  Every
 * product and sum is rounded once and none is contracted, in BOTH libraries: the values are the reference's doubles bit for
 * bit (tests/test_gpu_intpol.py, tests/test_gpu_intpol_exact.py), which is what lets a host writer switch to this call without
 * a byte of its files changing.  Times outside [time0, time1] extrapolate as the formula gives.
 *   Not-finite inputs (this project's definition: the reference's FMOD casts to int, which is undefined there): a point
 * whose time, lon or lat -- or p, when a pressure-level field is requested -- is not finite, or whose |lon| > 1e9, gets NaN
 * in every requested field.
 *   Refused, nothing written to out, the cause in mphip_last_error: a slot without a snapshot; time0 == time1; n < 0; ntime
 * not 1 or n; a NULL lon, lat, out, time or field; a NULL p with a pressure-level field; nfield outside 1 ... 32; a field
 * index out of range; a model-level field (MPHIP_PL, UL, VL, WL, ZETAL, ZETA_DOTL: another level count, out of scope); a
 * field that either resident snapshot was uploaded without (the message names the field); a grid whose three axes hold
 * more than 4096 nodes together (the kernel keeps them in 64 KB of LDS, 16 bytes per node). */
#define MPHIP_INTPOL_2D 256   /* flag bit above MPHIP_N3D */
int mphip_intpol_met(mphip_ctx *ctx, long long n, const double *time, long long ntime, const double *p, const double *lon,
                     const double *lat, int nfield, const int *field, double *out);

/* mptrac_update_device(..., atm), mptrac.c:8050-8055.  This process owns the
 * particles [ip0, ip0 + np) of a simulation with np_total particles; random
 * numbers are drawn for the global index so results do not depend on the
 * sharding.  q[iq] may be NULL for iq >= nq. */
int mphip_update_atm(mphip_ctx *ctx, long long np, long long ip0, long long np_total, int nq,
                     const double *time, const double *p, const double *lon, const double *lat,
                     const double *const *q);
/* One quantity array of the particles, in the caller's order: for a host-side writer that changes a single
 * quantity of the model state (write_station sets the station flag, mptrac.c:15143-15145 -- on the reference's
 * CPU path that is the state the next time step sees). */
int mphip_update_quantity(mphip_ctx *ctx, int iq, const double *q);
/* mptrac_update_host(..., atm), mptrac.c:8105-8110 */
int mphip_get_atm(mphip_ctx *ctx, double *time, double *p, double *lon, double *lat,
                  double *const *q);
/* mptrac_update_device / _host (cache), mptrac.c:8020-8025, 8076-8081, plus the
 * file-static rng_ctr (mptrac.c:35).  uvwp is [np][3] as cache_t
 * (mptrac.h:3633); any pointer may be NULL. */
int mphip_update_cache(mphip_ctx *ctx, const float *uvwp, const uint64_t *rng_ctr);
int mphip_get_cache(mphip_ctx *ctx, float *uvwp, double *dt, uint64_t *rng_ctr);
/* The isosurface part of cache_t (iso_var[np], iso_ts / iso_ps [iso_n]; mptrac.h:3620-3632), as
 * mptrac_update_device / _host move it.  iso_var (per particle slot; filled on the device by
 * module_isosurf_init for ISOSURF 1-3) and the balloon time series read by module_isosurf_init for
 * ISOSURF 4 (mptrac.c:4925-4951); any pointer may be NULL. */
int mphip_update_iso(mphip_ctx *ctx, const double *iso_var, const double *iso_ts, const double *iso_ps, int iso_n);
int mphip_get_iso(mphip_ctx *ctx, double *iso_var);

/* mptrac_run_timestep, mptrac.c:7851-8001: the reference's module order and
 * gating, fused into as few launches as the order allows. */
/* module_mixing (mptrac.c:5169-5347) mixes the quantities of the hot path -- mass, volume mixing ratio, the trace
 * gases, age of air (qnt_m, qnt_vmr, qnt_tracer, qnt_aoa) -- and the radionuclide activities registered with
 * mphip_set_radio_decay, in one pass; each quantity mixes on its own.  The other quantities of the reference's list
 * (mptrac.c:5223-5230) are left untouched. */
int mphip_run_timestep(mphip_ctx *ctx, double t);
/* The time loop of the reference's driver (trac.c:204-226: `for (t = t_start; ...; t += direction * dt_mod)
 * mptrac_run_timestep(...)`) for `nsteps` consecutive steps starting at t_first: same results as nsteps calls of
 * mphip_run_timestep.  Steps with nothing scheduled between them may share one kernel launch (option
 * "multi_step" = most steps per launch, default 64; 0 = never) -- what small particle counts need, where a time
 * step is shorter than a launch.  A driver calls it for the steps up to its next output.
 * What shares launches: every integrator (ADVECT 1 / 2 / 4) and every subset of turbulent / mesoscale diffusion,
 * convection, sedimentation, with the loss / decay / deposition modules and boundary conditions, on pressure and on
 * model levels.  A step at which module_sort, module_mixing or (CONV_DT > 0) module_convection is due runs on its own
 * and a batch ends before it; module_meteo is deferred as in mphip_run_timestep, so a batch ends only behind a step that
 * schedules it when the next one does not.  module_isosurf and the boundary-layer closure (TURB_PBL_SCHEME 1) share
 * launches on pressure-level winds.  Single steps throughout: the first step (t == T_START), ADVECT 0, ISOSURF or
 * TURB_PBL_SCHEME 1 with winds from the model levels, the option "generic_kernel", module_oh_chem (OH_CHEM_REACTION
 * != 0: a kernel of its own between module_mixing and module_wet_depo), module_chem_grid and module_h2o2_chem (with
 * either chemistry on: kernels of their own in the same place, in the order chem_grid, oh_chem, h2o2_chem),
 * module_tracer_chem (TRACER_CHEM != 0: a kernel of its own behind them and before module_wet_depo).
 * module_radio_decay (mphip_set_radio_decay) is no obstacle: it runs in the tail of the step kernel.  module_radio_depo
 * (mphip_set_radio_depo, on with a depositing activity and a deposition module): a launch of its own behind the tail. */
int mphip_run_timesteps(mphip_ctx *ctx, double t_first, int nsteps);
/* One reference module_* on its own (same state hand-over through the device
 * copy of cache->dt); `modules` is one MPHIP_MOD_* bit or an OR of the
 * per-particle bits in reference order (MPHIP_MOD_RADIO_DECAY counts as one of them). */
int mphip_module(mphip_ctx *ctx, unsigned modules, double t);
/* Keys (as the reference's double keys) and permutation of the last
 * module_sort call, for order checks. */
int mphip_get_sort(mphip_ctx *ctx, double *keys, int *perm);
/* How the module_sort calls of this context were answered so far: *repaired by the repair of the previous order
 * (option "sort_repair": the sort ahead of a step whose particles are stored in the order of the last module_sort),
 * *scratch by the radix sort of all pairs; *undone (may be NULL): those of *scratch that found the particles stored in
 * the internal locality order and restored the caller's order first.  Host counters, read-only; calls on an empty
 * particle set count as none of them. */
int mphip_get_sort_counts(mphip_ctx *ctx, long long *repaired, long long *scratch, long long *undone);

/* write_grid's binning loop (mptrac.c:13815-13872) on the device: cnt[ncell],
 * mean[nq][ncell], sigma[nq][ncell] raw sums (added in ascending particle index like the reference's loop,
 * option "deterministic_sums"), summed over the ranks through the communicator or the all-reduce hook if
 * one is set. */
int mphip_grid_sums(mphip_ctx *ctx, double t, int *cnt, double *mean, double *sigma);
/* The vertical weighting function of write_grid (GRID_KERNEL; read_kernel + kernel_weight, mptrac.c:8846-8883,
 * 3298-3320, used at mptrac.c:13866): nk nodes (height [km] ascending, weight -- already scaled to a largest
 * weight of one as read_kernel does); every summand of mphip_grid_sums is then kernel * q (and its square).
 * nk < 2 switches it off (weight one, the default). */
int mphip_set_grid_kernel(mphip_ctx *ctx, int nk, const double *kz, const double *kw);
/* The particle loops of the four analysis outputs that look at every particle in every time step, on the device (the
 * reference's writers run them on the host behind mptrac_update_host, src/mptrac.c write_csi, write_prof, write_sample,
 * write_station; here: mptrac_amd/host/output.c, whose loops these calls reproduce bit for bit -- same decisions, sums
 * added in ascending particle index).  All three need MET_COORD_TYPE 0 and work on the resident particles in the
 * caller's (external) index order whatever the internal storage order is.
 *
 * A regular longitude / latitude / log-pressure-height box grid (upper bounds exclusive). */
typedef struct {
  double lon0, lon1;
  int nx;
  double lat0, lat1;
  int ny;
  double z0, z1;
  int nz;
} mphip_box_t;
/* write_csi's and write_prof's binning loops (output.c:377-387, 557-563): for every particle with
 * t - dt_mod / 2 <= time <= t + dt_mod / 2 and member = (int) q[qnt_member] (0 when qnt_member < 0, which needs
 * nmember == 1): a member outside [0, nmember) is an error ("Ensemble ID out of range!" with the particle's index;
 * checked before the box test), else with c = box of (lon, lat, Z(p)): sum[member * ncell + c] += kernel_weight(p) *
 * q[qnt], ncell = nx ny nz, the summands of a cell in ascending particle index.  nk nodes (kz ascending, kw) of the
 * vertical weighting function as read_kernel leaves them; nk < 2: weight one.  sum[nmember * ncell] are raw sums, summed
 * over the ranks through the communicator or the all-reduce hook like mphip_grid_sums. */
int mphip_box_sums(mphip_ctx *ctx, const mphip_box_t *box, double t, int qnt, int nmember, int qnt_member, int nk,
                   const double *kz, const double *kw, double *sum);
/* write_sample's inner loop (output.c:640-652) for the nobs observations of a time step: count[i] = particles with
 * t0 <= time <= t1, fabs(obs_lat[i] - lat) <= dx 180 / (pi RE), dist2(geo2cart(observation), geo2cart(particle)) <= dx^2
 * and -- when dz > 0 -- P(obs_z[i] + dz) <= p <= P(obs_z[i] - dz); mass[i] = sum of kernel_weight(p) * q[qnt_m] over them
 * in ascending particle index (zeros without a quantity m; mass may be NULL).  dx [km], dz [km], the kernel as in
 * mphip_box_sums.  Counts and masses are summed over the ranks like the box sums. */
int mphip_sample_obs(mphip_ctx *ctx, double t0, double t1, int nobs, const double *obs_lon, const double *obs_lat,
                     const double *obs_z, double dx, double dz, int nk, const double *kz, const double *kw, int *count,
                     double *mass);
/* write_station's loop (output.c:696-714): the particles with time inside the time step around t and inside
 * [stat_t0, stat_t1], within r [km] of the station at (lon, lat) -- dist2 of the Cartesian positions against r^2 --, in
 * ascending particle index: *nhit of them, index[k] and rows[k][4 + nq] = time, p, lon, lat, q[0 .. nq).  qnt_stat >= 0:
 * particles whose flag (int) q[qnt_stat] is set are skipped, and the flag of the listed ones is set to 1 on the device
 * (rows show it as 1) -- no mphip_update_quantity afterwards.  *nhit > cap: nothing else is returned and no flag has
 * changed; call again with larger buffers.  One process only (the reference's write_station runs on rank 0 with all
 * particles): refused with a communicator or an index range that is not the whole simulation. */
int mphip_station_hits(mphip_ctx *ctx, double t, double lon, double lat, double r, double stat_t0, double stat_t1,
                       int qnt_stat, int cap, int *nhit, int *index, double *rows);
/* A read-only selection of the resident particles in the caller's (external) order: what a strided, windowed or boxed
 * writer needs of mphip_get_atm without taking all of it (write_atm_asc with ATM_STRIDE / ATM_FILTER 2, write_vtk).
 *   An external index e (rank-local, as in mphip_get_atm) is a candidate when first <= e <= last and
 * (e - first) % stride == 0; a candidate is selected when no enabled criterion rejects it (all criteria are ANDed).
 * Every test has the negated-or form written beside the members below, the form of write_atm_asc and of the box test of
 * the analysis outputs: a NaN coordinate therefore PASSES the range it is tested against (and the distance test).  A
 * caller who wants `time >= t0 && time <= t1` drops the NaN times from the few rows it gets back.  Z(p) is the
 * log-pressure height of mptrac.h:2243 with the C library's log (restated on the device; both libraries decide alike);
 * the distance test is the station loop's: geo2cart of the particle at the surface against that of the centre (the
 * host's C library), squared distance against near_r^2.  Longitudes are compared as stored, without wrapping. */
typedef struct {
  long long first, last;   /* external (caller-order, rank-local) indices considered: first <= e <= last;
                              last < 0 or last >= np: np - 1 */
  long long stride;        /* >= 1; e is a candidate when (e - first) % stride == 0 */
  int use_time, use_z, use_lon, use_lat, use_near;
  double t0, t1;           /* rejected when time < t0 || time > t1 */
  double z0, z1;           /* rejected when Z(p) < z0 || Z(p) > z1, Z as in mptrac.h:2243 */
  double lon0, lon1;       /* rejected when lon < lon0 || lon > lon1 (stored longitude, no wrap) */
  double lat0, lat1;       /* rejected when lat < lat0 || lat > lat1 */
  double near_lon, near_lat, near_r;   /* km; rejected when |geo2cart(0, lon, lat) - geo2cart(0, near_lon, near_lat)|^2 > near_r^2 */
} mphip_select_t;
/* The selected particles in ascending external index: *nsel of them, index[k] the external index, time[k], p[k], lon[k],
 * lat[k], q[iq][k] its values -- the bits mphip_get_atm delivers at that index.  Any output pointer, q itself and any
 * q[iq] may be NULL: that row is neither gathered nor copied.  Every array given holds cap elements.  *nsel > cap:
 * nothing but *nsel is written and the call returns 0; call again with larger arrays (cap = 0 counts only).  np == 0 or
 * first > last: *nsel = 0.
 *   The call only reads: a pending deferred module_meteo is flushed first, as in mphip_get_atm, and neither the stored
 * order nor any particle value changes, so a time loop with calls in between has the bits of one without.  It works on a
 * context that is one rank of several; nothing is reduced.  Beyond the marks (4 bytes per particle, twice) device memory
 * grows with *nsel only: the two lists and two rows of doubles, whatever nq is.
 *   Refused, with a message that names the call and nothing written: NULL ctx, sel or nsel; stride < 1, first < 0,
 * cap < 0; an enabled range with a NaN bound or a lower bound above the upper; near_r negative or not finite; use_lon,
 * use_lat or use_near on a Cartesian grid (met_coord_type != 0; use_time and use_z work there, as write_atm_asc does);
 * control parameters not uploaded. */
int mphip_select_atm(mphip_ctx *ctx, const mphip_select_t *sel, long long cap, long long *nsel, int *index, double *time,
                     double *p, double *lon, double *lat, double *const *q);
/* module_radio_decay (RADIO_DECAY): qnt[MPHIP_RN_*] is the quantity index of each activity [Bq] (-1: absent).  The
 * registered activities are mixed by module_mixing whether or not the module is on.  on != 0: mphip_run_timestep(s)
 * decay them after module_decay, module_mixing and the chemistry and before module_wet_depo, in the step kernel's tail
 * (steps with it still share multi-step launches); for every particle with dt != 0 and each present activity
 * A *= exp(-lambda dt), and Pb-210 gains the ingrowth of the Rn-222 it had before the step (two-member Bateman solution;
 * lambda = ln 2 / half-life).  mphip_module(ctx, MPHIP_MOD_RADIO_DECAY, t) runs it alone on the stored dt.  Refused:
 * an index outside [0, nq), one index twice, an index that is m, vmr, a loss quantity, aoa, a trace gas, Cx or a
 * module_meteo quantity (also when mphip_update_ctl later makes it one).  qnt may be NULL when on == 0: nothing
 * registered. */
int mphip_set_radio_decay(mphip_ctx *ctx, int on, const int qnt[MPHIP_NRADIO]);
/* module_radio_depo (RADIO_DEPO; the reference's depo_t): the activity module_wet_depo and module_dry_depo take out of the
 * air, and a gridded inventory of where it lands.  The reference's source was not available (as for the half-lives of
 * module_radio_decay): what follows is this project's own definition, restated in tests/refradiodepo.py.
 *   The ground grid is the longitude / latitude part of `grid` (nz must be 1; z0, z1 are ignored), ncell = nx ny.  The
 * inventory is inv[2][MPHIP_NRADIO][ncell + 1] [Bq]: kind 0 wet, 1 dry; nuclides in MPHIP_RN_* order; cell ix ny + iy with
 * the arithmetic of mphip_box_sums' boxes (upper bounds exclusive); the last element of every plane collects the deposits
 * outside the grid.  The aerosol-bound Apb210, Abe7, Acs137, Ai131 deposit; the noble gases Arn222 and Axe133 never do --
 * their planes and those of absent activities stay zero.
 *   on != 0: in a time step at t (mphip_run_timestep(s)) with a depositing activity registered (mphip_set_radio_decay) and
 * module_wet_depo or module_dry_depo configured, a launch behind the step's tail (1) decays the inventory on the ground:
 * every element of nuclide k times exp(-lambda_k (t - t_inv)), the C library's exp, then t_inv = t (the first step only
 * sets t_inv; no ingrowth on the ground: Rn-222 is never deposited); (2) for every particle with dt != 0, at its final
 * position, takes the factors aux_w, aux_d = exp(-dt lambda) of the two deposition modules as the tail applied them to m
 * (same switches, early-outs and operands) and, for every depositing present activity, a1 = a0 aux_w, w = a0 - a1 if the
 * wet module acts, then a2 = a1 aux_d, d = a1 - a2 if the dry module acts, A = a2 -- every product and difference rounded
 * once in both libraries, so the deposit is the activity before minus the activity after bit for bit; (3) adds the w and d
 * of all particles per cell in ascending external particle index (no floating-point atomics; the result does not depend
 * on the stored order, which the locality re-sort changes; module_sort redefines the external order itself and with it the
 * order of summation, so a cell with three or more deposits may round differently with SORT_DT set) and sets
 * inv = inv f + step, two roundings.  m, vmr, the loss quantities, positions, cache and random-number
 * counters are what they are without the module.  Such steps share no multi-step launch.
 * mphip_module(ctx, MPHIP_MOD_RADIO_DEPO, t) runs the module alone on the stored dt.
 *   mphip_set_radio_depo with a new grid allocates the inventory, zeroes it and forgets t_inv; with the same grid it keeps
 * the inventory (on toggled).  grid may be NULL when on == 0.  Refused: nz != 1, an empty or inverted grid, ncell + 1
 * beyond 32-bit cell indices; with on != 0 also DIRECTION != 1, MET_COORD_TYPE != 0, no depositing activity registered
 * (and mphip_update_ctl / mphip_set_radio_decay refuse to create these conditions while it is on).  The launch needs the
 * lean deposition code -- a regular longitude / latitude meteo grid whose packed records fit 32-bit offsets, option
 * "generic_kernel" off -- and refuses the step otherwise.
 *   mphip_get_radio_depo: t_inv (NaN before the first step) and the planes wet, dry [MPHIP_NRADIO][ncell + 1] (any
 * pointer may be NULL), summed over the ranks through the communicator or the all-reduce hook like mphip_grid_sums (every
 * rank keeps the deposits of its own particles: no exchange inside the step).  Refused before mphip_set_radio_depo. */
int mphip_set_radio_depo(mphip_ctx *ctx, int on, const mphip_box_t *grid);
int mphip_get_radio_depo(mphip_ctx *ctx, double *t_inv, double *wet, double *dry);

int mphip_set_allreduce(mphip_ctx *ctx, mphip_allreduce_fn fn, void *user);

/* Multi-GPU without a host language in the data path: one process per GPU, every process owns one context
 * with an index range of the particles (mphip_update_atm: ip0, np_total) and the same meteo data.  The only
 * exchanges are the cell sums of module_mixing (mptrac.c:5289-5316: one grouped all-reduce per mixing step --
 * the sums of all mixed quantities as doubles, the cell counts once as 32-bit integers) and write_grid's sums
 * (mptrac.c:13862-13872).  With a communicator they are RCCL all-reduces issued on the context's own stream;
 * the host thread never waits for them.  librccl is loaded with dlopen at the first call, single-GPU callers
 * do not need it.  Replaces the rank -> device binding of the reference's driver (src/trac.c:70-81).
 *   mphip_comm_unique_id: rank 0 creates the 128-byte identifier (ncclGetUniqueId) and hands it to the other
 *     ranks by whatever the host has (MPI_Bcast, a TCP socket as host/trac.c does, torch.distributed);
 *   mphip_comm_init: collective over all ranks (ncclCommInitRank), after hipSetDevice of mphip_create;
 *   mphip_comm_destroy: back to a single rank (mphip_destroy does it too).
 * A communicator takes precedence over an all-reduce hook. */
int mphip_comm_unique_id(void *id128);
int mphip_comm_init(mphip_ctx *ctx, int nranks, int rank, const void *id128);
int mphip_comm_destroy(mphip_ctx *ctx);
/* What the communicator itself reports (ncclCommCount / ncclCommUserRank): *nranks = 0 without a communicator.
 * A launcher prints it next to its results so that a run that was meant to span N GPUs can be told from N
 * independent ones (the reference prints its MPI rank / size the same way, trac.c:70-81). */
int mphip_comm_query(mphip_ctx *ctx, int *nranks, int *rank);

/* Tuning knobs without a reference counterpart.
 *   "locality_sort_interval" (default 60): the device keeps the particles stored
 *   in meteo-grid-cell order and re-sorts every this many time steps so that
 *   the gathers of neighbouring particles share cache lines.  The order is
 *   internal: random numbers follow the external slot index and every download
 *   returns the caller's order, so results do not depend on the value.
 *   0 switches it off.
 *   "locality_tile" (default 0 = 4, or 8 with model-level winds): edge, in grid columns, of the horizontal tiles of
 *   that order (tile, then level, then column within the tile).
 *   "step_blocks" (default 8192): upper bound of the step kernel's grid;
 *   "xcd_map" (default 1): give each XCD one contiguous eighth of the particles;
 *   "step_queue" (default 1): the step kernel runs as a grid that is resident at once (at most step_blocks /
 *   step_blocks_multi workgroups) whose waves claim chunks of 64 particles from one queue per XCD ("xcd_map" 0: from
 *   one queue) and, once their own is used up, from the others -- in launches with 16 chunks or more per wave of
 *   that grid (4.2 million particles on an MI355X: below, the queues' fixed cost per launch outweighs the shorter
 *   tail); 2 = in every launch; 0 = never: every workgroup walks its fixed share of the particles.  Results do not
 *   depend on the value;
 *   "lazy_meteo" (default 1): module_meteo (mptrac.c:7921-7924) writes quantities
 *   no module reads, so the launch a time step schedules is held back until
 *   its result can be seen -- mphip_get_atm, mphip_grid_sums, mphip_module --
 *   or its inputs change (meteo / control uploads), and is dropped when the
 *   next time step would overwrite it unseen; a time step that does not run
 *   module_meteo evaluates a pending one first, before the particles move.
 *   Downloads are bit-identical either way.  0 = launch it inside every step;
 *   "fuse_sort" (default 1): inside mphip_run_timestep the gather of time, p,
 *   lon, lat that module_sort ends with (mptrac.c:5944-5949) happens in the step
 *   launch that follows; 0 = every array is re-ordered in module_sort's own pass;
 *   "fold_resort" (default 1): inside mphip_run_timesteps, a re-sort of the internal locality order that falls due
 *   with at least two steps to share a launch behind it (pressure-level winds, a lean multi-step kernel for the
 *   module set, no module_isosurf) has no gather pass of its own: the launch reads the particles through the sort's
 *   permutation and takes the due step with the others; 0 = the re-sort gathers in its own pass and its step is a
 *   launch of its own, as in mphip_run_timestep.  Not observable;
 *   "turb_strat" (default 1): module_diff_turb in the lean kernels with 32-bit offsets: a wavefront whose particles all
 *   lie above the boundary layer and above 0.866877899 x the smallest tropopause pressure the climatology can give at
 *   any time and any latitude in [-90, 90] (1 % margin; with TURB_DX_STRAT 0, finite parameters >= 0, MET_COORD_TYPE
 *   0) takes the stratosphere's TURB_DZ_STRAT directly, without the tropopause look-up, the weights and the first pair
 *   of normals; 0 = every wavefront evaluates them.  Not observable;
 *   "pin_host_atm" (default 0): page-lock the caller's particle arrays handed to
 *   mphip_update_atm / mphip_get_atm with one registration spanning them (for
 *   a persistent atm_t whose arrays lie in one allocation);
 *   "deterministic_sums" (default 1): the cell sums of module_mixing and of mphip_grid_sums add every cell's
 *   summands in ascending particle index, as the reference's serial loops do (mptrac.c:5289-5303,
 *   13862-13872): same bits as the serial code, from run to run and for any storage order.  0 = floating-point
 *   atomics (order of arrival; faster when single cells hold very many particles);
 *   "sort_bits" (default 0 = the width with the fewest passes; 8, 9, 10): digit width of the radix sort;
 *   "compact_depo" (default 1): a launch of module_wet_depo / module_dry_depo alone (what follows module_mixing in
 *   a time step) first packs the particles with anything to do into full waves; 0 = tail of the fused kernel.
 *   Not observable;
 *   "sort_ahead" (default 1): keys, module_timesteps and radix sort of the next time step's module_sort start on a
 *   second stream as soon as this step's particles have moved, beside module_mixing and the deposition modules;
 *   taken over by the next mphip_run_timestep if it comes with the expected time and nothing they depend on was
 *   touched in between, dropped otherwise.  Not observable;
 *   "grid_records" (default 1): mphip_grid_sums first interleaves the quantities of every particle into one record
 *   (one pass), so that the ordered sums pull one or two cache lines per particle instead of one per quantity;
 *   0 = gather from the quantity arrays.  Not observable;
 *   "locality_zorder" (default 0): number the tiles of the internal order along a Z-order curve instead of row by
 *   row (measured: no effect on the step kernel);
 *   "sum_path" (default 0 = by crowding; 1, 2): tests -- force the group / the chain algorithm of the ordered sums;
 *   "chain_blocks": tuning -- workgroups of the chain walk of the ordered sums;
 *   "generic_kernel" (default 0): tuning aid, never pick a specialised kernel;
 *   "mix_exchange_levels" (default 0): with several ranks, exchange the cell sums of module_mixing only for the band of
 *     grid levels that holds particles on any rank (a small all-reduce of the per-level occupancy, read by the host, then
 *     the band); same results, a third of the bytes on the default grid, one host synchronisation per mixing step;
 *   "lds_tile" (default 0 = off; 64 ... 2400): cells of an LDS tile of wind records that runs of pure trajectory steps
 *     (mphip_run_timesteps with module_timesteps, module_position, module_advect only) stage per workgroup; same results,
 *     measured slower than the default gathers;
 *   "emit_keys" (default 1): in a time step with module_mixing, the launch that moves the particles also writes the keys
 *     of the next step's module_sort, its module_timesteps and module_mixing's box index (otherwise a kernel of their own
 *     behind it); same values.  Taken for the headline module set only -- ADVECT 4 with turbulent + mesoscale diffusion,
 *     convection and sedimentation, no module_bound_cond; every other set (ADVECT 2 / 1, subsets of the movers, the
 *     boundary condition) keeps the separate key kernel;
 *   "sort_repair" (default 1): the module_sort that runs ahead repairs the order of the previous module_sort (only the
 *     particles that changed their cell are sorted, then merged with the others) instead of sorting from scratch; same
 *     permutation
 *   "big_grid" (default 0): tests -- take the instantiations with 64-bit byte offsets into the packed meteo records (what a
 *     grid with more than 4 GB of wind records -- 178e6 cells -- takes by itself) on a grid that fits 32 bits too: same bits.
 *   "derive_profile_phase" (default 0; 1 ... 6): measurement -- what mphip_profile_begin / _end time of a mphip_derive_met
 *     call: every kernel (0), the uploads (1) or the downloads (2), as event pairs on the call's own stream (a caller that
 *     profiles does not step from another thread meanwhile); 3: the host's build of the weight table in
 *     mphip_detrend_met (the stream is idle meanwhile, so the pair of events brackets the host's time); 4, 5, 6: of the
 *     kernels of mphip_pack_met only the extremes, their reduction, the quantisation (mphip_unpack_met and mphip_pack_met
 *     are calls of the same family: 0, 1 and 2 hold for them as well).
 *   "intpol_chunk" (default 4194304 = 2^22; 64 ... 16777216 = 2^24): points per launch of mphip_intpol_met -- its two
 *     device buffers hold 32 + 8 nfield bytes per point of a chunk.  Not observable.
 *   "select_direct" (default 0): mphip_select_atm copies every gathered row straight into the caller's array (page-locked
 *     in one span under "pin_host_atm", as mphip_get_atm has them) instead of through the context's two page-locked rows.
 *     Not observable.
 *   "select_profile_phase" (default 0; 1 ... 5): measurement -- what mphip_profile_begin / _end time of a
 *     mphip_select_atm call: every kernel (0), or only the mark kernel (1), the scan (2), the list kernel (3), the row
 *     gathers (4), the copies to the host (5). */
int mphip_set_option(mphip_ctx *ctx, const char *name, double value);
int mphip_synchronize(mphip_ctx *ctx);

/* The bounds of the four early exits as the next launch would use them, from the two uploaded snapshots and the control
 * parameters: bounds[0] ps_skip (module_dry_depo returns for p < ps_skip - DRY_DEPO_DP), [1] pct_skip (module_wet_depo
 * for p <= pct_skip), [2] turb_skip (module_diff_turb: no boundary layer for 1.01 p < turb_skip), [3] conv_skip
 * (module_convection for p < conv_skip); each only for a particle time between the snapshots.  -inf: that exit is never
 * taken -- a field value that is not finite, no control parameters yet, or a grid on which the reference's horizontal
 * weights can leave [0, 1]: a longitude / latitude grid whose longitude axis spans less than 360 degrees or starts
 * outside [-360, 0] (intpol_check_lon_lat shifts a longitude by one period and never clamps it, so beyond such an axis
 * the interpolation extrapolates below every node value).  A longitude axis that passes for periodic (|span - 360| <
 * 0.01) and still spans less than 360 loses the exits too; mphip_update_met says so once on stderr. */
int mphip_get_shortcuts(mphip_ctx *ctx, double bounds[4]);

/* Timing of the fused step kernel with HIP events on the context's stream:
 * between begin and end every launch is bracketed; end returns the launch
 * count and the summed device time. */
int mphip_profile_begin(mphip_ctx *ctx);
int mphip_profile_end(mphip_ctx *ctx, long long *launches, double *kernel_ms);

/* Device self-tests used by tests/ (single-precision sine/cosine of the
 * Box-Muller step over a range of float bit patterns; uniform and normal
 * random numbers for given counters). */
int mphip_test_sincosf(mphip_ctx *ctx, uint32_t bits_first, uint32_t count, float *cos_out,
                       float *sin_out);
int mphip_test_rng(mphip_ctx *ctx, uint64_t ctr, long long n, int method, double *out);
/* out[i] = exp(x[i]) (op 0), log(x[i]) (1), pow(x[i], y[i]) (2), sqrt(x[i]) (3), cos(x[i]) (4), sin(x[i]) (5) as the
 * kernels evaluate them: the restatement of the C library's exp / log / pow the reference's CPU build links
 * (src/mptrac.c:4531-4546, 5822; csrc/mphip_libm.h), the square root of the Box-Muller radius, and the library's
 * cos / sin of DX2DEG / ZETA (mptrac.h:904, 2293; the reference-rounding build and module_meteo), op 6 / 7: the cos / sin
 * of geo2cart in the analysis outputs (the library's bits for |x| < 105414350); op + 16 reads the exp / log / pow tables
 * from an LDS copy.
 * x, y, out are host arrays of n doubles. */
int mphip_test_libm(mphip_ctx *ctx, int op, const double *x, const double *y, long long n, double *out);
/* Profiling aid: run building block `piece` of the step kernel (stencil set-up, one Runge-Kutta stage's
 * interpolation, the random-number triple, ...; list in mphip_kernels.hpp:piece_kernel) `reps` times per
 * resident particle; tools/piece_cost.py reads the instruction counters of these launches. */
int mphip_test_piece(mphip_ctx *ctx, int piece, int reps, double *checksum);
/* The table of module_diff_meso's wind deviations of the current meteo pair -- {sd_u, sd_v, sd_w} per raw grid cell,
 * what the lean kernels read instead of summing the cell's 16 wind values per particle and step (mptrac.c:4287-4318) --
 * in plain order: out[((ix (ny - 1) + iy) (np - 1) + ip) 3 + k], cells = (nx - 1) (ny - 1) (np - 1).  Builds the table
 * if the current packed grids have none. */
int mphip_test_meso_table(mphip_ctx *ctx, float *out, size_t cells);
#ifdef __cplusplus
}
#endif
#endif
