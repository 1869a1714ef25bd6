// mphip_metprep.hpp -- the derived fields of the reference's meteo preprocessing (geopotential height, total ozone
// column, boundary-layer pressure, cloud layer, CAPE, potential vorticity, tropopause) from one snapshot "as stored",
// column-parallel on the device (the smoothing and the potential vorticity: tiled stencils): the kernels behind
// mphip_derive_met.
//
// The definitions are this project's own statement of the reference's algorithms (include/mptrac_hip.h, at
// mphip_derive_met; restated independently in tests/refmetprep.py and tests/reftropo.py): the reference's source was
// not available, so no line of mptrac.c is cited for them.  All arithmetic is in double from the float inputs and every
// output value is rounded to float once.
//
// Layout.  The fields are [ix][iy][ip] with ip fastest.  A lane that walked its column in global memory would stride
// np floats across the wave, so a workgroup (one wave) first copies the columns it owns -- they are contiguous -- into
// LDS with coalesced loads, at a row pitch of np | 1 floats (odd: the 64 lanes of a walk hit 64 different banks), and
// one lane then walks one column.  Workgroups of one wave own 64 columns, or the largest power of two below whose
// fields fit 64 KB (DESIGN.md section 7 on the choice).
//
// Every loop below ends by construction: a level loop runs over at most np levels, the bisection halves a finite
// interval, the parcel's pressure shrinks by pfac per pass, and the tropopause searches count a fine-grid index up to
// kTropoTop; a NaN makes each loop condition false.  (An infinite
// surface pressure would not: it is taken as NaN.)
#pragma once

#include "mphip_device.hpp"

namespace mphip {

constexpr double kPrepMO3 = 48.00;                  // molar mass of ozone [g/mol]
constexpr double kPrepZD = kRI / kMA / kG0;         // RI / MA / G0: km per K and unit of log-pressure
constexpr double kPrepPfac = 1.01439;               // pressure ratio of one pass of the parcel ascent
constexpr int kPrepLanes = 64;

struct PrepGrid {
  int nx, ny, np;
  int cpb;              // columns per workgroup (a power of two, <= 64)
  int pitch;            // LDS row pitch [floats]: np | 1
  int ncol;             // nx * ny
  const double *p;      // pressure axis [np], strictly descending
  const double *lat;    // latitudes [ny]
};

// what the column kernels need beside the fields
struct PrepOpt {
  int met_pbl;
  double pbl_min, pbl_max, cloud_min;
  double time;          // of the snapshot (tropopause climatology)
  int coord_type;
  double ref_lat;       // met_utm_ref_lat: the latitude of the tropopause on a Cartesian grid
};

__device__ __forceinline__ float prep_nanf() {
  return __builtin_nanf("");
}

__device__ __forceinline__ double prep_nan() {
  return __builtin_nan("");
}

__device__ __forceinline__ double prep_ps(float ps) {   // (see the note on loops above)
  const double v = (double) ps;
  return fabs(v) == __builtin_inf() ? prep_nan() : v;
}

// LDS of a column workgroup: double p[np], lp[np] (log p, geopotential only), then nf float planes [cpb][pitch]
__device__ __forceinline__ double *prep_axis(const PrepGrid &G, double *smem, bool with_log) {
  for (int k = threadIdx.x; k < G.np; k += blockDim.x) {
    smem[k] = G.p[k];
    if (with_log)
      smem[G.np + k] = libm_log(G.p[k]);
  }
  return smem;
}

__device__ __forceinline__ float *prep_planes(const PrepGrid &G, double *smem) {
  return (float *) (smem + 2 * (size_t) G.np);
}

// columns [col0, col0 + ncols) of a compact field -> plane; a field that is absent (NULL) reads as zero
__device__ __forceinline__ void prep_stage(const PrepGrid &G, float *plane, const float *__restrict__ src, int col0, int ncols) {
  const int n = ncols * G.np;
  const float *s = src ? src + (size_t) col0 * (size_t) G.np : nullptr;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int c = i / G.np, k = i - c * G.np;
    plane[c * G.pitch + k] = s ? s[i] : 0.f;
  }
}

__device__ __forceinline__ int prep_ncols(const PrepGrid &G, int col0) {
  const int left = G.ncol - col0;
  return left < G.cpb ? left : G.cpb;
}

// loc(q): the largest k in [0, np - 2] with p[k] >= q, else 0 (p descending: a walk from `from`, which must not lie
// above the result -- 0, or the result for a larger q)
__device__ __forceinline__ int prep_loc(const double *pa, int np, double q, int from = 0) {
  int k = from;
  while (k < np - 2 && pa[k + 1] >= q)
    k++;
  return k;
}

__device__ __forceinline__ double prep_pz(double z) {   // P(z)
  return kP0 * libm_exp(-z / kH0);
}

__device__ __forceinline__ double prep_zd(double a, double ta, double b, double tb) {
  return kPrepZD * (0.5 * (ta + tb)) * (a - b);
}

// ---- geopotential height [km], before the smoothing ---------------------------------------------------------------
__global__ __launch_bounds__(kPrepLanes) void prep_geopot_kernel(const PrepGrid G, const float *__restrict__ t,
                                                                 const float *__restrict__ h2o, const float *__restrict__ ps2,
                                                                 const float *__restrict__ zs2, float *__restrict__ zout) {
  extern __shared__ double prep_smem[];
  const int col0 = blockIdx.x * G.cpb, ncols = prep_ncols(G, col0), np = G.np;
  const double *pa = prep_axis(G, prep_smem, true), *lp = pa + np;
  float *tc = prep_planes(G, prep_smem), *hc = tc + (size_t) G.cpb * G.pitch, *zc = hc + (size_t) G.cpb * G.pitch;
  prep_stage(G, tc, t, col0, ncols);
  prep_stage(G, hc, h2o, col0, ncols);
  __syncthreads();
  if ((int) threadIdx.x < ncols) {
    const float *tl = tc + threadIdx.x * G.pitch, *hl = hc + threadIdx.x * G.pitch;
    float *zl = zc + threadIdx.x * G.pitch;
    const double ps = prep_ps(ps2[col0 + threadIdx.x]), zs = (double) zs2[col0 + threadIdx.x];
    const int k0 = prep_loc(pa, np, ps);
    const double tv0 = tvirt(tl[k0], hl[k0]), tv1 = tvirt(tl[k0 + 1], hl[k0 + 1]);
    const double tsurf = lin_nodes(pa[k0], tv0, pa[k0 + 1], tv1, ps), lps = libm_log(ps);
    double z = zs + prep_zd(lps, tsurf, lp[k0 + 1], tv1), tv_prev = tv1;
    zl[k0 + 1] = (float) z;
    for (int k = k0 + 2; k < np; k++) {
      const double tv = tvirt(tl[k], hl[k]);
      z = z + prep_zd(lp[k - 1], tv_prev, lp[k], tv);
      zl[k] = (float) z;
      tv_prev = tv;
    }
    z = zs + prep_zd(lps, tsurf, lp[k0], tv0);
    zl[k0] = (float) z;
    tv_prev = tv0;
    for (int k = k0 - 1; k >= 0; k--) {
      const double tv = tvirt(tl[k], hl[k]);
      z = z + prep_zd(lp[k + 1], tv_prev, lp[k], tv);
      zl[k] = (float) z;
      tv_prev = tv;
    }
  }
  __syncthreads();
  const int n = ncols * np;
  float *dst = zout + (size_t) col0 * (size_t) np;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int c = i / np, k = i - c * np;
    dst[i] = zc[c * G.pitch + k];
  }
}

// ---- horizontal smoothing of the float field, per level -----------------------------------------------------------
// A workgroup owns a tile of kSmTX x kSmTY columns and kSmKC levels; it copies the tile and its halo of sx - 1 / sy - 1
// columns into LDS (the longitude index wrapped once by +-nx, on regional grids too; what lies outside the latitude
// range or the grid reads as NaN, which the sum over finite values skips like the clamped loop bounds of the
// definition), 16 consecutive levels of a column per 64-byte segment, and every thread then sums four columns of one
// level: float weights, float sums of w z and w in the order ix2 (outer), iy2 (inner), uncontracted.
constexpr int kSmTX = 8, kSmTY = 8, kSmKC = 16;

__global__ __launch_bounds__(256) void prep_smooth_kernel(const PrepGrid G, int sx, int sy, const float *__restrict__ zin,
                                                          float *__restrict__ zout) {
#pragma clang fp contract(off)
  extern __shared__ float prep_tile[];
  const int hx_n = kSmTX + 2 * (sx - 1), hy_n = kSmTY + 2 * (sy - 1);
  const int ix0 = blockIdx.x * kSmTX, iy0 = blockIdx.y * kSmTY, k0 = blockIdx.z * kSmKC;
  const int n = hx_n * hy_n * kSmKC;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int k = i % kSmKC, hy = (i / kSmKC) % hy_n, hx = i / (kSmKC * hy_n);
    int ix2 = ix0 - (sx - 1) + hx;
    const int iy2 = iy0 - (sy - 1) + hy, kk = k0 + k;
    if (ix2 < 0)
      ix2 += G.nx;
    else if (ix2 >= G.nx)
      ix2 -= G.nx;
    const bool inside = ix2 >= 0 && ix2 < G.nx && iy2 >= 0 && iy2 < G.ny && kk < G.np;
    prep_tile[i] = inside ? zin[((size_t) ix2 * G.ny + iy2) * (size_t) G.np + kk] : prep_nanf();
  }
  __syncthreads();
  const int k = threadIdx.x % kSmKC, kk = k0 + k;
  const float fsx = (float) sx, fsy = (float) sy;
  for (int c = threadIdx.x / kSmKC; c < kSmTX * kSmTY; c += 256 / kSmKC) {
    const int tx = c / kSmTY, ty = c % kSmTY, ix = ix0 + tx, iy = iy0 + ty;
    if (ix >= G.nx || iy >= G.ny || kk >= G.np)
      continue;
    float ws = 0.f, wz = 0.f;
    for (int dx = 0; dx < 2 * sx - 1; dx++) {
      const float wx = 1.0f - (float) abs(dx - (sx - 1)) / fsx;
      for (int dy = 0; dy < 2 * sy - 1; dy++) {
        const float v = prep_tile[((tx + dx) * hy_n + (ty + dy)) * kSmKC + k];
        if (!(fabsf(v) < __builtin_inff()))
          continue;
        const float w = wx * (1.0f - (float) abs(dy - (sy - 1)) / fsy);
        const float prod = w * v;
        wz = wz + prod;
        ws = ws + w;
      }
    }
    zout[((size_t) ix * G.ny + iy) * (size_t) G.np + kk] = ws > 0.f ? wz / ws : prep_nanf();
  }
}

// ---- total ozone column [DU] --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPrepLanes) void prep_o3c_kernel(const PrepGrid G, const float *__restrict__ o3,
                                                              const float *__restrict__ ps2, float *__restrict__ o3c) {
  extern __shared__ double prep_smem[];
  const int col0 = blockIdx.x * G.cpb, ncols = prep_ncols(G, col0), np = G.np;
  const double *pa = prep_axis(G, prep_smem, false);
  float *oc = prep_planes(G, prep_smem);
  prep_stage(G, oc, o3, col0, ncols);
  __syncthreads();
  if ((int) threadIdx.x >= ncols)
    return;
  const float *ol = oc + threadIdx.x * G.pitch;
  const double ps = (double) ps2[col0 + threadIdx.x];
  double cd = 0;
  for (int k = 1; k < np; k++)
    if (pa[k - 1] <= ps)
      cd += 0.5 * ((double) ol[k - 1] + (double) ol[k]) * kPrepMO3 / kMA * (pa[k - 1] - pa[k]) * 100. / kG0;
  o3c[col0 + threadIdx.x] = (float) (cd / 2.1415e-5);
}

// ---- cloud layer: top and bottom pressure [hPa], total column cloud water [kg/m^2] -------------------------------------
__global__ __launch_bounds__(kPrepLanes) void prep_cloud_kernel(const PrepGrid G, const PrepOpt O, const float *__restrict__ lwc,
                                                                const float *__restrict__ rwc, const float *__restrict__ iwc,
                                                                const float *__restrict__ swc, const float *__restrict__ ps2,
                                                                float *__restrict__ pct, float *__restrict__ pcb,
                                                                float *__restrict__ cl) {
  extern __shared__ double prep_smem[];
  const int col0 = blockIdx.x * G.cpb, ncols = prep_ncols(G, col0), np = G.np;
  const double *pa = prep_axis(G, prep_smem, false);
  const size_t plane = (size_t) G.cpb * G.pitch;
  float *f0 = prep_planes(G, prep_smem);
  prep_stage(G, f0, lwc, col0, ncols);
  prep_stage(G, f0 + plane, rwc, col0, ncols);
  prep_stage(G, f0 + 2 * plane, iwc, col0, ncols);
  prep_stage(G, f0 + 3 * plane, swc, col0, ncols);
  __syncthreads();
  if ((int) threadIdx.x >= ncols)
    return;
  const float *l = f0 + threadIdx.x * G.pitch, *r = l + plane, *i = r + plane, *s = i + plane;
  const double ps = (double) ps2[col0 + threadIdx.x], p20 = prep_pz(20.);
  double top = prep_nan(), bot = prep_nan(), col = 0;
  for (int k = 0; k < np - 1; k++) {
    if (pa[k] > ps || pa[k] < p20)
      continue;
    if (l[k] > O.cloud_min || r[k] > O.cloud_min || i[k] > O.cloud_min || s[k] > O.cloud_min) {
      top = 0.5 * (pa[k] + pa[k + 1]);
      if (!(bot == bot))
        bot = 0.5 * (pa[k] + pa[k > 0 ? k - 1 : 0]);
    }
    const double sum = (((double) l[k] + (double) l[k + 1]) + ((double) r[k] + (double) r[k + 1]))
      + ((double) i[k] + (double) i[k + 1]) + ((double) s[k] + (double) s[k + 1]);
    col += 0.5 * sum * 100. * (pa[k] - pa[k + 1]) / kG0;
  }
  pct[col0 + threadIdx.x] = (float) top;
  pcb[col0 + threadIdx.x] = (float) bot;
  cl[col0 + threadIdx.x] = (float) col;
}

// ---- boundary-layer pressure [hPa] --------------------------------------------------------------------------------------
__device__ __forceinline__ double prep_pbl_clamp(const PrepOpt &O, double ps, double pbl, bool below_surface) {
  const double pmin = ps * libm_exp(-O.pbl_min / kH0), pmax = ps * libm_exp(-O.pbl_max / kH0);
  if (!(fabs(pbl) < __builtin_inf()) || pbl > pmin || below_surface)
    pbl = pmin;
  if (pbl < pmax)
    pbl = pmax;
  return pbl;
}

// met_pbl 3 stages t; met_pbl 2 stages t, h2o, u, v, z
__global__ __launch_bounds__(kPrepLanes) void prep_pbl_kernel(const PrepGrid G, const PrepOpt O, const float *__restrict__ t,
                                                              const float *__restrict__ h2o, const float *__restrict__ u,
                                                              const float *__restrict__ v, const float *__restrict__ z,
                                                              const float *__restrict__ ps2, const float *__restrict__ ts2,
                                                              const float *__restrict__ zs2, const float *__restrict__ us2,
                                                              const float *__restrict__ vs2, float *__restrict__ pbl_out) {
  extern __shared__ double prep_smem[];
  const int col0 = blockIdx.x * G.cpb, ncols = prep_ncols(G, col0), np = G.np;
  const double *pa = prep_axis(G, prep_smem, false);
  const size_t plane = (size_t) G.cpb * G.pitch;
  float *f0 = prep_planes(G, prep_smem);
  prep_stage(G, f0, t, col0, ncols);
  if (O.met_pbl == 2) {
    prep_stage(G, f0 + plane, h2o, col0, ncols);
    prep_stage(G, f0 + 2 * plane, u, col0, ncols);
    prep_stage(G, f0 + 3 * plane, v, col0, ncols);
    prep_stage(G, f0 + 4 * plane, z, col0, ncols);
  }
  __syncthreads();
  if ((int) threadIdx.x >= ncols)
    return;
  const int col = col0 + threadIdx.x;
  const float *tl = f0 + threadIdx.x * G.pitch;
  const double ps = (double) ps2[col], ts = (double) ts2[col];
  double pbl;
  if (O.met_pbl == 3) {
    const double th0 = theta_of(ps, ts);
    int k = np - 2;
    for (; k > 0; k--)
      if (pa[k] >= 300. && (pa[k] > ps || theta_of(pa[k], tl[k]) <= th0 + 2.))
        break;
    pbl = lin_nodes(theta_of(pa[k + 1], tl[k + 1]), pa[k + 1], theta_of(pa[k], tl[k]), pa[k], th0 + 2.);
    pbl = prep_pbl_clamp(O, ps, pbl, pa[k] > ps);
  } else {
    const float *hl = tl + plane, *ul = hl + plane, *vl = ul + plane, *zl = vl + plane;
    const double zs = (double) zs2[col], us = (double) us2[col], vs = (double) vs2[col];
    const double pb = ps * libm_exp(-0.05 / kH0);
    int k = 1;
    while (k < np - 1 && !(pa[k] < pb))   // the first level >= 1 above pb (the last level if there is none)
      k++;
    const double h2os = lin_nodes(pa[k - 1], hl[k - 1], pa[k], hl[k], pb);
    const double tvs = tvirt(theta_of(pb, ts), h2os);
    double rib_old = 0;
    pbl = pb;
    for (; k < np; k++) {
      const double du = (double) ul[k] - us, dv = (double) vl[k] - vs;
      const double vh2 = dmax(du * du + dv * dv, 25.);
      const double rib = kG0 * 1e3 * ((double) zl[k] - zs) / tvs * (tvirt(theta_of(pa[k], tl[k]), hl[k]) - tvs) / vh2;
      if (rib >= 0.25) {
        pbl = dmin(lin_nodes(rib_old, pa[k - 1], rib, pa[k], 0.25), pb);
        break;
      }
      rib_old = rib;
    }
    pbl = prep_pbl_clamp(O, ps, pbl, false);
  }
  pbl_out[col] = (float) pbl;
}

// ---- CAPE, CIN [J/kg], lifted condensation level, level of free convection, equilibrium level [hPa] ----------------------
__device__ __forceinline__ double prep_env(const double *pa, const float *f, int k, double q) {
  return lin_nodes(pa[k], (double) f[k], pa[k + 1], (double) f[k + 1], q);
}

__global__ __launch_bounds__(kPrepLanes) void prep_cape_kernel(const PrepGrid G, const PrepOpt O, const DevClim *__restrict__ clim,
                                                               const float *__restrict__ t, const float *__restrict__ h2o,
                                                               const float *__restrict__ ps2, float *__restrict__ plcl_out,
                                                               float *__restrict__ plfc_out, float *__restrict__ pel_out,
                                                               float *__restrict__ cape_out, float *__restrict__ cin_out) {
  extern __shared__ double prep_smem[];
  const int col0 = blockIdx.x * G.cpb, ncols = prep_ncols(G, col0), np = G.np;
  const double *pa = prep_axis(G, prep_smem, false);
  float *tc = prep_planes(G, prep_smem), *hc = tc + (size_t) G.cpb * G.pitch;
  prep_stage(G, tc, t, col0, ncols);
  prep_stage(G, hc, h2o, col0, ncols);
  __syncthreads();
  if ((int) threadIdx.x >= ncols)
    return;
  const int col = col0 + threadIdx.x;
  const float *tl = tc + threadIdx.x * G.pitch, *hl = hc + threadIdx.x * G.pitch;
  const double ps = prep_ps(ps2[col]);
  double plcl = prep_nan(), plfc = prep_nan(), pel = prep_nan(), cape = prep_nan(), cin = prep_nan();
  // the parcel: mean potential temperature and water vapour of the lowest 50 hPa
  double pbot = dmin(ps, pa[0]), theta = 0, h2o_p = 0;
  int n = 0;
  for (int k = 0; k < np; k++) {
    if (pbot >= pa[k] && pa[k] >= pbot - 50.) {
      theta += theta_of(pa[k], tl[k]);
      h2o_p += (double) hl[k];
      n++;
    } else if (n > 0 && pa[k] < pbot - 50.)
      break;
  }
  if (n > 0) {
    theta /= n;
    h2o_p /= n;
  }
  if (n > 0 && !(h2o_p <= 0)) {
    // lifted condensation level: bisection on the relative humidity of the lifted parcel
    double ptop = prep_pz(20.), tp;
    pbot = ps;
    do {
      plcl = 0.5 * (pbot + ptop);
      tp = theta / libm_pow(1000. / plcl, kKappa);
      if (100. * pw_of(plcl, h2o_p) / psat_of(tp) > 100.)
        ptop = plcl;
      else
        pbot = plcl;
    } while (pbot - ptop > 0.1);
    // dry adiabat from the surface to the lifted condensation level
    const double dz0 = kPrepZD * libm_log(kPrepPfac);
    cape = cin = 0;
    double p = ps;
    int ke = 0;
    do {
      const double dz = dz0 * tvirt(tp, h2o_p);
      p /= kPrepPfac;
      tp = theta / libm_pow(1000. / p, kKappa);
      ke = prep_loc(pa, np, p, ke);
      const double tve = tvirt(prep_env(pa, tl, ke, p), prep_env(pa, hl, ke, p));
      const double d = 1e3 * kG0 * (tvirt(tp, h2o_p) - tve) / tve * dz;
      if (d < 0)
        cin += fabs(d);
    } while (p > plcl);
    // moist adiabat up to three quarters of the climatological tropopause pressure
    double d = 0;
    p = plcl;
    tp = theta / libm_pow(1000. / p, kKappa);
    ptop = 0.75 * clim_tropo(*clim, O.time, O.coord_type == 0 ? G.lat[col % G.ny] : O.ref_lat);
    ke = 0;
    do {
      const double dz = dz0 * tvirt(tp, h2o_p);
      p /= kPrepPfac;
      tp -= lapse_rate(tp, h2o_p) * dz;
      const double psat = psat_of(tp);
      h2o_p = psat / (p - (1. - kEps) * psat);
      ke = prep_loc(pa, np, p, ke);
      const double tve = tvirt(prep_env(pa, tl, ke, p), prep_env(pa, hl, ke, p));
      const double d_old = d;
      d = 1e3 * kG0 * (tvirt(tp, h2o_p) - tve) / tve * dz;
      if (d > 0) {
        cape += d;
        if (!(plfc == plfc))
          plfc = p;
      } else if (d_old > 0)
        pel = p;
      if (d < 0 && !(plfc == plfc))
        cin += fabs(d);
    } while (p > ptop && p > 0.);   // (p > 0: a top that is not positive -- no tropopause table has one -- still ends)
    if (!(plfc == plfc))
      cin = prep_nan();
  }
  plcl_out[col] = (float) plcl;
  plfc_out[col] = (float) plfc;
  pel_out[col] = (float) pel;
  cape_out[col] = (float) cape;
  cin_out[col] = (float) cin;
}

// ---- potential vorticity [PVU] --------------------------------------------------------------------------------------
// A workgroup owns a tile of kPvTX x kPvTY columns and kPvKC levels and copies t, u, v of the tile, of its halo of one
// column (indices clamped to the grid, as ix0 / ix1 / iy0 / iy1 of the definition are) and of one level below and above
// (clamped likewise: at an end level a[k0] or a[k1] is a[k] itself) into LDS: the 32 lanes of a half-wave load 34
// consecutive levels of a column, and every input is read from memory 1.66 times rather than five.  One thread per column
// then computes the six row quantities (three cosines and a sine) once for all levels; after that a lane is a level
// and a half-wave a column.  The rows next to the poles are overwritten by prep_pv_polar_kernel, launched behind this
// kernel on the same stream.
constexpr int kPvTX = 8, kPvTY = 8, kPvKC = 32, kPvPitch = kPvKC + 3, kPvCols = (kPvTX + 2) * (kPvTY + 2);
constexpr size_t kPvLds = (size_t) (2 * (kPvKC + 2) + 6 * kPvTX * kPvTY) * sizeof(double)
  + (size_t) 3 * kPvCols * kPvPitch * sizeof(float);

__device__ __forceinline__ double prep_rad(double x) {
  return x * (kPi / 180.0);
}

__device__ __forceinline__ int prep_clampi(int i, int hi) {
  return i < 0 ? 0 : (i > hi ? hi : i);
}

// d a / d p at a level: dp0 = 100 (p[k] - p[k0]), dp1 = 100 (p[k1] - p[k]); a0, a, a1 at k0, k, k1
__device__ __forceinline__ double prep_ddp(bool interior, double dp0, double dp1, double a0, double a, double a1) {
  if (interior)
    return (dp0 * dp0 * a1 - dp1 * dp1 * a0 + (dp1 * dp1 - dp0 * dp0) * a) / (dp0 * dp1 * (dp0 + dp1));
  return (a1 - a0) / (dp0 + dp1);
}

__global__ __launch_bounds__(256) void prep_pv_kernel(const PrepGrid G, const double *__restrict__ lon,
                                                      const double *__restrict__ pows, const float *__restrict__ t, const float *__restrict__ u,
                                                      const float *__restrict__ v, float *__restrict__ pv) {
  extern __shared__ double prep_smem[];
  constexpr int nl = kPvKC + 2, hy_n = kPvTY + 2;
  double *pa = prep_smem, *pw = pa + nl, *rq = pw + nl;      // p and pows of the levels k0 - 1 ... k0 + kPvKC; rq[column][6]
  float *tt = (float *) (rq + 6 * kPvTX * kPvTY), *ut = tt + kPvCols * kPvPitch, *vt = ut + kPvCols * kPvPitch;
  const int ix0 = blockIdx.x * kPvTX, iy0 = blockIdx.y * kPvTY, k0 = blockIdx.z * kPvKC;
  for (int l = threadIdx.x; l < nl; l += blockDim.x) {
    const int kk = prep_clampi(k0 - 1 + l, G.np - 1);
    pa[l] = G.p[kk];
    pw[l] = pows[kk];
  }
  for (int i = threadIdx.x; i < kPvCols * nl; i += blockDim.x) {
    const int c = i / nl, l = i - c * nl, hx = c / hy_n, hy = c - hx * hy_n;
    const int ix = prep_clampi(ix0 - 1 + hx, G.nx - 1), iy = prep_clampi(iy0 - 1 + hy, G.ny - 1);
    const size_t g = ((size_t) ix * G.ny + iy) * (size_t) G.np + prep_clampi(k0 - 1 + l, G.np - 1);
    tt[c * kPvPitch + l] = t[g];
    ut[c * kPvPitch + l] = u[g];
    vt[c * kPvPitch + l] = v[g];
  }
  if (threadIdx.x < kPvTX * kPvTY) {
    const int tx = threadIdx.x / kPvTY, ty = threadIdx.x % kPvTY, ix = ix0 + tx, iy = iy0 + ty;
    if (ix < G.nx && iy < G.ny) {
      const int xa = ix > 0 ? ix - 1 : 0, xb = ix < G.nx - 1 ? ix + 1 : G.nx - 1;
      const int ya = iy > 0 ? iy - 1 : 0, yb = iy < G.ny - 1 ? iy + 1 : G.ny - 1;
      const double latr = 0.5 * (G.lat[yb] + G.lat[ya]);
      const double cr = libm_cos(prep_rad(latr));
      double *r = rq + 6 * threadIdx.x;
      r[0] = 1000. * (kRE * prep_rad(lon[xb] - lon[xa]) * cr);      // dx
      r[1] = 1000. * (kRE * prep_rad(G.lat[yb] - G.lat[ya]));       // dy
      r[2] = libm_cos(prep_rad(G.lat[ya]));                         // c0
      r[3] = libm_cos(prep_rad(G.lat[yb]));                         // c1
      r[4] = cr;
      r[5] = 2 * 2 * kPi / 86400. * libm_sin(prep_rad(G.lat[iy]));  // vort
    }
  }
  __syncthreads();
  const int l = threadIdx.x % kPvKC + 1, kk = k0 + l - 1;
  if (kk >= G.np)
    return;
  const bool interior = kk > 0 && kk < G.np - 1;
  const double dp0 = 100. * (pa[l] - pa[l - 1]), dp1 = 100. * (pa[l + 1] - pa[l]);
  const double w0 = pw[l - 1], w = pw[l], w1 = pw[l + 1];
  for (int c = threadIdx.x / kPvKC; c < kPvTX * kPvTY; c += 256 / kPvKC) {
    const int tx = c / kPvTY, ty = c % kPvTY, ix = ix0 + tx, iy = iy0 + ty;
    if (ix >= G.nx || iy >= G.ny)
      continue;
    const double *r = rq + 6 * c;
    const double dx = r[0], dy = r[1], c0 = r[2], c1 = r[3], cr = r[4], vort = r[5];
    const int m = ((tx + 1) * hy_n + ty + 1) * kPvPitch + l;           // this column; its neighbours in x and y:
    const int xm = m - hy_n * kPvPitch, xp = m + hy_n * kPvPitch, ym = m - kPvPitch, yp = m + kPvPitch;
    const double dtdx = ((double) tt[xp] - (double) tt[xm]) * w / dx;
    const double dvdx = ((double) vt[xp] - (double) vt[xm]) / dx;
    const double dtdy = ((double) tt[yp] - (double) tt[ym]) * w / dy;
    const double dudy = ((double) ut[yp] * c1 - (double) ut[ym] * c0) / dy;
    const double dtdp = prep_ddp(interior, dp0, dp1, (double) tt[m - 1] * w0, (double) tt[m] * w, (double) tt[m + 1] * w1);
    const double dudp = prep_ddp(interior, dp0, dp1, (double) ut[m - 1], (double) ut[m], (double) ut[m + 1]);
    const double dvdp = prep_ddp(interior, dp0, dp1, (double) vt[m - 1], (double) vt[m], (double) vt[m + 1]);
    const double val = 1e6 * kG0 * (-dtdp * (dvdx - dudy / cr + vort) + dvdp * dtdx - dudp * dtdy);
    pv[((size_t) ix * G.ny + iy) * (size_t) G.np + kk] = (float) val;
  }
}

// rows 0 and 1 take row 2's value, rows ny - 1 and ny - 2 row ny - 3's (ny >= 5: no source row is a target)
__global__ __launch_bounds__(256) void prep_pv_polar_kernel(const PrepGrid G, float *__restrict__ pv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= G.nx * G.np)
    return;
  const int ix = i / G.np, k = i - ix * G.np;
  float *col = pv + (size_t) ix * G.ny * (size_t) G.np + k;
  const float lo = col[(size_t) 2 * G.np], hi = col[(size_t) (G.ny - 3) * G.np];
  col[0] = lo;
  col[G.np] = lo;
  col[(size_t) (G.ny - 1) * G.np] = hi;
  col[(size_t) (G.ny - 2) * G.np] = hi;
}

// ---- tropopause: pressure [hPa], temperature [K], geopotential height [km], water vapour [ppv] ---------------------------
// The fine grid z2[i] = 4.5 + 0.1 i km, p2 = P(z2), and what the natural cubic spline through a column profile on zc[k] =
// Z(p[k]) owes to the pressure axis alone -- the interval widths h, the factors w and the eliminated diagonal d of its
// tridiagonal system -- come from the host (PrepTropo::tab, behind the axes) and are copied to LDS once per workgroup; a
// lane solves only the right-hand side of its column (g -> c, in place) and evaluates.
constexpr int kTropoFine = 201, kTropoTop = 170;

struct PrepTropo {
  int mode, spline;          // met_tropo 1 ... 5; 1 = cubic, 0 = linear
  double pv_thr, theta_thr;
  int nprof;                 // staged float planes per column: 0 (mode 1), 1 (t), 2 (t, pv: mode 5)
  int fine;                  // doubles of the fine profile kept per column: kTropoFine (modes 3, 4) or 0
  const double *tab;         // zc[np] h[np] w[np] d[np] pows[np] z2[kTropoFine] p2[kTropoFine]
};

struct TropoLds {
  const double *p, *zc, *h, *w, *d, *pows, *z2, *p2;
};

// the spline through y(k) at z2[i]; k is the walk's state (start at 0, i ascending)
template <class Y> __device__ __forceinline__ double prep_spline_at(const TropoLds &L, int np, int method, const double *c,
                                                                    Y y, int i, int &k) {
  const double x = L.z2[i];
  if (x <= L.zc[0])
    return y(0);
  if (x >= L.zc[np - 1])
    return y(np - 1);
  while (k < np - 2 && L.zc[k + 1] <= x)
    k++;
  const double y0 = y(k), y1 = y(k + 1);
  if (method == 0)
    return lin_nodes(L.zc[k], y0, L.zc[k + 1], y1, x);
  const double h = L.h[k];
  const double b = (y1 - y0) / h - h * (c[k + 1] + 2 * c[k]) / 3;
  const double e = (c[k + 1] - c[k]) / (3 * h);
  const double dx = x - L.zc[k];
  return y0 + dx * (b + dx * (c[k] + dx * e));
}

// second-derivative coefficients c[0 ... np-1] of the natural cubic spline through y(k)
template <class Y> __device__ __forceinline__ void prep_spline_solve(const TropoLds &L, int np, double *c, Y y) {
  c[0] = c[np - 1] = 0;
  double gprev = 0;
  for (int i = 0; i <= np - 3; i++) {
    double g = 3 * ((y(i + 2) - y(i + 1)) / L.h[i + 1] - (y(i + 1) - y(i)) / L.h[i]);
    if (i > 0)
      g -= L.w[i] * gprev;
    c[i + 1] = gprev = g;
  }
  c[np - 2] = c[np - 2] / L.d[np - 3];
  for (int i = np - 4; i >= 0; i--)
    c[i + 1] = (c[i + 1] - L.h[i + 1] * c[i + 2]) / L.d[i];
}

__device__ __forceinline__ double prep_lapse(double p1, double t1, double p2, double t2) {
  return 1e3 * kG0 / kRA * (t2 - t1) / (t2 + t1) * (p2 + p1) / (p2 - p1);
}

// B(iz): the lapse rate to each of the next n fine points is <= 2 K/km (WMO); A(iz): >= 3 K/km
__device__ __forceinline__ bool prep_wmo(const double *p2, const double *t2, int iz, int n, bool second) {
  for (int j = iz + 1; j <= iz + n; j++) {
    const double g = prep_lapse(p2[iz], t2[iz], p2[j], t2[j]);
    if (second ? !(g >= 3.0) : !(g <= 2.0))
      return false;
  }
  return true;
}

__global__ __launch_bounds__(kPrepLanes) void prep_tropo_kernel(const PrepGrid G, const PrepOpt O, const PrepTropo T,
                                                                const DevClim *__restrict__ clim, const float *__restrict__ t,
                                                                const float *__restrict__ h2o, const float *__restrict__ z,
                                                                const float *__restrict__ pvf, float *__restrict__ pt_out,
                                                                float *__restrict__ tt_out, float *__restrict__ zt_out,
                                                                float *__restrict__ h2ot_out) {
  extern __shared__ double prep_smem[];
  const int col0 = blockIdx.x * G.cpb, ncols = prep_ncols(G, col0), np = G.np;
  const int ntab = 5 * np + 2 * kTropoFine;
  for (int k = threadIdx.x; k < np; k += blockDim.x)
    prep_smem[k] = G.p[k];
  if (T.mode != 1)
    for (int k = threadIdx.x; k < ntab; k += blockDim.x)
      prep_smem[np + k] = T.tab[k];
  TropoLds L;
  L.p = prep_smem;
  L.zc = L.p + np;
  L.h = L.zc + np;
  L.w = L.h + np;
  L.d = L.w + np;
  L.pows = L.d + np;
  L.z2 = L.pows + np;
  L.p2 = L.z2 + kTropoFine;
  double *dcol = prep_smem + np + ntab;                       // per column: c[np], then the fine profile
  const int dper = np + T.fine;
  float *f0 = (float *) (dcol + (size_t) G.cpb * dper);
  const size_t plane = (size_t) G.cpb * G.pitch;
  if (T.nprof > 0)
    prep_stage(G, f0, t, col0, ncols);
  if (T.nprof > 1)
    prep_stage(G, f0 + plane, pvf, col0, ncols);
  __syncthreads();
  if ((int) threadIdx.x >= ncols)
    return;
  const int col = col0 + threadIdx.x;
  const float *tl = f0 + threadIdx.x * G.pitch, *pl = tl + plane;
  double *c = dcol + (size_t) threadIdx.x * dper, *t2 = c + np;
  const auto yt = [&](int k) { return (double) tl[k]; };
  const auto yp = [&](int k) { return (double) pl[k]; };
  const auto yth = [&](int k) { return (double) tl[k] * L.pows[k]; };
  double pt = prep_nan();
  bool bad = false;
  if (T.mode == 1)
    pt = clim_tropo(*clim, O.time, O.coord_type == 0 ? G.lat[col % G.ny] : O.ref_lat);
  else if (T.mode == 2) {
    if (T.spline)
      prep_spline_solve(L, np, c, yt);
    int k = 0, iz = 0;
    double tmin = 0;
    for (int i = 0; i <= kTropoTop; i++) {
      const double v = prep_spline_at(L, np, T.spline, c, yt, i, k);
      bad = bad || !(v == v);
      if (i == 0 || v < tmin) {
        tmin = v;
        iz = i;
      }
    }
    if (!bad && iz > 0 && iz < kTropoTop)
      pt = L.p2[iz];
  } else if (T.mode == 3 || T.mode == 4) {
    if (T.spline)
      prep_spline_solve(L, np, c, yt);
    int k = 0;
    for (int i = 0; i < kTropoFine; i++) {
      const double v = prep_spline_at(L, np, T.spline, c, yt, i, k);
      bad = bad || !(v == v);
      t2[i] = v;
    }
    int iz = 0;
    while (iz <= kTropoTop && !prep_wmo(L.p2, t2, iz, 20, false))
      iz++;
    if (T.mode == 4 && iz <= kTropoTop) {
      while (iz <= kTropoTop && !prep_wmo(L.p2, t2, iz, 10, true))
        iz++;
      while (iz <= kTropoTop && !prep_wmo(L.p2, t2, iz, 20, false))
        iz++;
    }
    if (!bad && iz > 0 && iz < kTropoTop)
      pt = L.p2[iz];
  } else {
    // two splines share c: the potential vorticity first, then the potential temperature; the first hit of either decides
    int hit = kTropoTop + 1, k = 0;
    if (T.spline)
      prep_spline_solve(L, np, c, yp);
    for (int i = 0; i <= kTropoTop; i++) {
      const double v = prep_spline_at(L, np, T.spline, c, yp, i, k);
      bad = bad || !(v == v);
      if (hit > kTropoTop && fabs(v) >= T.pv_thr)
        hit = i;
    }
    if (T.spline)
      prep_spline_solve(L, np, c, yth);
    k = 0;
    for (int i = 0; i <= kTropoTop; i++) {
      const double v = prep_spline_at(L, np, T.spline, c, yth, i, k);
      bad = bad || !(v == v);
      if (i < hit && v >= T.theta_thr)
        hit = i;
    }
    if (!bad && hit > 0 && hit < kTropoTop)
      pt = L.p2[hit];
  }
  double tt = prep_nan(), zt = prep_nan(), ht = prep_nan();
  if (pt == pt) {
    const int k = prep_loc(L.p, np, pt);
    const size_t g = (size_t) col * (size_t) np + k;
    tt = lin_nodes(L.p[k], (double) t[g], L.p[k + 1], (double) t[g + 1], pt);
    zt = lin_nodes(L.p[k], (double) z[g], L.p[k + 1], (double) z[g + 1], pt);
    ht = lin_nodes(L.p[k], (double) h2o[g], L.p[k + 1], (double) h2o[g + 1], pt);
  }
  pt_out[col] = (float) pt;
  tt_out[col] = (float) tt;
  zt_out[col] = (float) zt;
  h2ot_out[col] = (float) ht;
}

}   // namespace mphip
