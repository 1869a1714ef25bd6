// mphip_intpol.hpp -- mphip_intpol_met: the resident meteo pair interpolated at the caller's points
// (intpol_met_time_3d / intpol_met_time_2d of the reference, mptrac.c:2755-3170; the definition: include/mptrac_hip.h).
//
// Both builds of the library return the reference's doubles bit for bit: every function below switches contraction
// off and divides with a plain `/` (an IEEE division in either build), so the weights are true quotients and every
// blend is a rounded product followed by a rounded sum.  That is a property of this call -- a host writer may take its
// values where the host interpolation's went without a byte of its files changing --, not of stencil_3d, whose weights
// are products with reciprocals in the default build; only the exact index helpers (locate_irr, locate_reg) are shared
// with the step kernels.
//
// Not-finite inputs (this project's definition; the reference's FMOD casts to int, which is undefined there): a point
// whose time, lon or lat -- or p, when a pressure-level field is requested -- is not finite, or whose |lon| > 1e9, gets
// NaN in every requested field.
#pragma once

#include "mphip_device.hpp"

namespace mphip {

constexpr int kIntpolMaxFields = 32;
constexpr int kIntpol2D = 1 << 8;        // MPHIP_INTPOL_2D: the field index names a surface field

struct IntpolArgs {
  const double *time, *p, *lon, *lat;    // the chunk's points (time: one per point, or NULL with time_all)
  double time_all;                       // the one time of all points (time == NULL)
  long long n;
  double *out;                           // [nfield][out_stride]
  long long out_stride;
  int nfield, need_p;
  int field[kIntpolMaxFields];           // MPHIP_* index, | kIntpol2D for a surface field
  const float *f0[kIntpolMaxFields];     // the field's staging copy of met0 / met1: [ix][iy][ip] or [ix][iy]
  const float *f1[kIntpolMaxFields];
};

// FMOD, mptrac.h:1121-1122, with the product rounded before the difference
__device__ __forceinline__ double intpol_fmod(double x, double y) {
#pragma clang fp contract(off)
  return x - (int) (x / y) * y;
}

__device__ __forceinline__ bool intpol_finite(double x) {
  return fabs(x) <= 1.7976931348623157e308;   // false for NaN
}

// intpol_check_lon_lat / intpol_check_cartesian, mptrac.c:2755-2803
__device__ __forceinline__ void intpol_check(const DevMet &M, const Axes &A, double lon, double lat, double &lon2,
                                             double &lat2) {
#pragma clang fp contract(off)
  const double x0 = A.lon[0], x1 = A.lon[M.nx - 1];
  const double y0 = A.lat[0], y1 = A.lat[M.ny - 1];
  if (M.coord_type == 0) {
    lon2 = intpol_fmod(lon, 360.);
    if (lon2 < x0)
      lon2 += 360;
    else if (lon2 > x1)
      lon2 -= 360;
  } else if (x0 < x1)
    lon2 = dmin(dmax(lon, x0), x1);
  else
    lon2 = dmin(dmax(lon, x1), x0);
  if (y0 < y1)
    lat2 = dmin(dmax(lat, y0), y1);
  else
    lat2 = dmin(dmax(lat, y1), y0);
}

// intpol_met_space_3d's blends (mptrac.c:3023-3044): vertical, then latitude, then longitude.  a[2 c] / a[2 c + 1]
// are the levels ip / ip + 1 of corner c = 2 (ix offset) + (iy offset).
__device__ __forceinline__ double intpol_blend_3d(const float *a, double wp, double wx, double wy) {
#pragma clang fp contract(off)
  // (the difference of the two levels is the reference's float difference, widened afterwards)
  const double c00 = wp * (double) (a[0] - a[1]) + (double) a[1];
  const double c01 = wp * (double) (a[2] - a[3]) + (double) a[3];
  const double c10 = wp * (double) (a[4] - a[5]) + (double) a[5];
  const double c11 = wp * (double) (a[6] - a[7]) + (double) a[7];
  const double r0 = wy * (c00 - c01) + c01;
  const double r1 = wy * (c10 - c11) + c11;
  return wx * (r0 - r1) + r1;
}

// intpol_met_space_2d's value (mptrac.c:3083-3108): bilinear, or the nearest corner if one is not finite
__device__ __forceinline__ double intpol_blend_2d(const float *a, double wx, double wy) {
#pragma clang fp contract(off)
  const double c00 = a[0], c01 = a[1], c10 = a[2], c11 = a[3];
  if (intpol_finite(c00) && intpol_finite(c01) && intpol_finite(c10) && intpol_finite(c11)) {
    const double r0 = wy * (c00 - c01) + c01;
    const double r1 = wy * (c10 - c11) + c11;
    return wx * (r0 - r1) + r1;
  }
  if (wy < 0.5)
    return wx < 0.5 ? c11 : c01;
  return wx < 0.5 ? c10 : c00;
}

// One lane per point.  The index and weight set is built once per point from met0's axes (LDS copy) and shared by all
// fields, as INTPOL_TIME_ALL does; the loop over the fields is wave-uniform, its pointers come from the kernel
// arguments.  Every index lies inside the grid whatever the point is: locate_irr returns 0 ... n - 2 for any x (a NaN
// included), locate_reg clamps, and a point that the not-finite rule refuses is searched with the first nodes.
__global__ __launch_bounds__(256) void intpol_points_kernel(DevMet M, IntpolArgs I) {
#pragma clang fp contract(off)
  extern __shared__ double s_axes[];
  const Axes A = load_axes(M, s_axes);
  __syncthreads();
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const size_t snp = (size_t) M.np, sny = (size_t) M.ny;
  for (long long i = blockIdx.x * (long long) blockDim.x + threadIdx.x; i < I.n; i += (long long) gridDim.x * blockDim.x) {
    double ts = I.time ? I.time[i] : I.time_all;
    double lon = I.lon[i], lat = I.lat[i];
    double p = I.need_p ? I.p[i] : A.p[0];
    const bool bad = !intpol_finite(ts) || !intpol_finite(lon) || !intpol_finite(lat) || !intpol_finite(p) || fabs(lon) > 1e9;
    if (bad) {
      ts = M.time0;
      lon = A.lon[0];
      lat = A.lat[0];
      p = A.p[0];
    }
    double lon2, lat2;
    intpol_check(M, A, lon, lat, lon2, lat2);
    const int ip = locate_irr(A.p, M.np, p, M.p_ascending);
    const int ix = locate_reg(A.lon, M.nx, lon2);
    const int iy = locate_irr(A.lat, M.ny, lat2, M.lat_ascending);
    const double wp = (A.p[ip + 1] - p) / (A.p[ip + 1] - A.p[ip]);
    const double wx = (A.lon[ix + 1] - lon2) / (A.lon[ix + 1] - A.lon[ix]);
    const double wy = (A.lat[iy + 1] - lat2) / (A.lat[iy + 1] - A.lat[iy]);
    const double wt = (M.time1 - ts) / (M.time1 - M.time0);
    const size_t col = (size_t) ix * sny + (size_t) iy;
    for (int k = 0; k < I.nfield; k++) {
      const float *__restrict__ g0 = I.f0[k];
      const float *__restrict__ g1 = I.f1[k];
      double v;
      if (I.field[k] & kIntpol2D) {
        float a[4], b[4];
        const size_t o[4] = { col, col + 1, col + sny, col + sny + 1 };
        for (int c = 0; c < 4; c++) {
          a[c] = g0[o[c]];
          b[c] = g1[o[c]];
        }
        const double v0 = intpol_blend_2d(a, wx, wy), v1 = intpol_blend_2d(b, wx, wy);
        if (intpol_finite(v0) && intpol_finite(v1))
          v = wt * (v0 - v1) + v1;
        else
          v = wt < 0.5 ? v1 : v0;
      } else {
        float a[8], b[8];
        const size_t c00 = col * snp + (size_t) ip;
        const size_t o[4] = { c00, c00 + snp, c00 + sny * snp, c00 + sny * snp + snp };
        for (int c = 0; c < 4; c++) {   // the two levels of a corner are neighbours in memory
          a[2 * c] = g0[o[c]];
          a[2 * c + 1] = g0[o[c] + 1];
          b[2 * c] = g1[o[c]];
          b[2 * c + 1] = g1[o[c] + 1];
        }
        const double v0 = intpol_blend_3d(a, wp, wx, wy), v1 = intpol_blend_3d(b, wp, wx, wy);
        v = wt * (v0 - v1) + v1;
      }
      I.out[(size_t) k * (size_t) I.out_stride + (size_t) i] = bad ? nan : v;
    }
  }
}

}   // namespace mphip
