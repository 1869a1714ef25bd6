// mphip_regrid.hpp -- the two grid-changing steps of the reference's meteo preprocessing: model levels to pressure
// levels (read_met_ml2pl) and smoothing with down-sampling (read_met_sample): the kernels behind mphip_regrid_met.
//
// The definitions are this project's own statement (include/mptrac_hip.h, at mphip_regrid_met; restated independently
// in tests/refregrid.py).  ML2PL interpolates in double and rounds each value to float once; SAMPLE is float
// arithmetic in a fixed order, never contracted.
//
// Layout.  The fields are [ix][iy][ip] with ip fastest, as in mphip_metprep.hpp.
//   ML2PL: a workgroup stages the model-level pressure of up to 64 consecutive columns in LDS (coalesced loads, row
// pitch npl | 1 floats: columns of one level lie on different banks) and the target pressures beside them; a lane owns
// one (column, target level) pair, clamps the target and bisects its column once and then interpolates every present
// field with that bracket.  Consecutive lanes own consecutive targets of one column: their stores are consecutive
// floats, and their two loads per field fall into a few cache lines of a column the workgroup reads completely.
//   SAMPLE: a workgroup owns a tile of kRgTX x kRgTY kept columns and KC kept levels.  It copies what their windows
// read into LDS -- per axis the window of a kept point starts min(stride, 2 s - 1) entries behind its neighbour's, so
// windows that overlap share their entries and windows that a large stride pulls apart are packed -- and a thread then
// sums the window of one kept point of four columns.  Only kept points are computed.
#pragma once

#include "mphip_device.hpp"

namespace mphip {

constexpr int kRgFields = 11;          // t, u, v, w, h2o, o3, lwc, rwc, iwc, swc, cc
constexpr int kRgThreads = 256;
constexpr int kRgTX = 8, kRgTY = 8, kRgKC = 16;

struct RegridFields {
  int n;
  const float *in[kRgFields];
  float *out[kRgFields];
};

// ---- model levels -> pressure levels ----------------------------------------------------------------------------------
// LDS: double q[mnp], then float pl[cpb][pitch]
__global__ __launch_bounds__(kRgThreads) void regrid_ml2pl_kernel(int ncol, int npl, int mnp, int cpb, int pitch,
                                                                  const double *__restrict__ met_p,
                                                                  const float *__restrict__ pl, const RegridFields F) {
  extern __shared__ double rg_smem[];
  double *qa = rg_smem;
  float *plc = (float *) (rg_smem + mnp);
  const int col0 = blockIdx.x * cpb, left = ncol - col0, ncols = left < cpb ? left : cpb;
  for (int j = threadIdx.x; j < mnp; j += blockDim.x)
    qa[j] = met_p[j];
  const float *src = pl + (size_t) col0 * (size_t) npl;
  for (int i = threadIdx.x; i < ncols * npl; i += blockDim.x) {
    const int c = i / npl, k = i - c * npl;
    plc[c * pitch + k] = src[i];
  }
  __syncthreads();
  const int n = npl, npairs = ncols * mnp;
  for (int i = threadIdx.x; i < npairs; i += blockDim.x) {
    const int c = i / mnp, j = i - c * mnp;
    const float *col = plc + c * pitch;
    double q = qa[j];
    const double p0 = (double) col[0], p1 = (double) col[1], pe = (double) col[n - 1];
    if (p0 > p1) {
      if (q > p0)
        q = p0;
      else if (q < pe)
        q = pe;
    } else {
      if (q < p0)
        q = p0;
      else if (q > pe)
        q = pe;
    }
    // locate_irr: the loop halves ihi - ilo, so it ends whatever the comparisons give
    int ilo = 0, ihi = n - 1, m = (ihi + ilo) >> 1;
    if ((double) col[m] < (double) col[m + 1]) {
      while (ihi > ilo + 1) {
        m = (ihi + ilo) >> 1;
        if ((double) col[m] > q)
          ihi = m;
        else
          ilo = m;
      }
    } else {
      while (ihi > ilo + 1) {
        m = (ihi + ilo) >> 1;
        if ((double) col[m] <= q)
          ihi = m;
        else
          ilo = m;
      }
    }
    const int k = ilo;
    const double x0 = (double) col[k], x1 = (double) col[k + 1];
    const size_t at = (size_t) (col0 + c) * (size_t) npl + k, to = (size_t) col0 * (size_t) mnp + i;
    for (int f = 0; f < F.n; f++) {
      const double y0 = (double) F.in[f][at], y1 = (double) F.in[f][at + 1];
      F.out[f][to] = (float) lin_nodes(x0, y0, x1, y1, q);
    }
  }
}

// ---- smoothing and down-sampling ---------------------------------------------------------------------------------------
struct RegridSample {
  int nx, ny, np;         // input extents (np = 1: a 2-D field)
  int nx2, ny2, np2;      // kept points
  int dx, dy, dp;         // strides
  int sx, sy, sp;         // half-widths
  int ex, ey, ep;         // LDS entries between the windows of neighbouring kept points: min(stride, 2 s - 1)
  int hx, hy, hk;         // LDS extents: (tile - 1) e + 2 s - 1
};

// input index of LDS entry h of a tile whose first kept point is o0 (tile points per axis: nt)
__device__ __forceinline__ int regrid_src(int h, int e, int nt, int o0, int d, int s) {
  int t = h / e;
  t = t < nt - 1 ? t : nt - 1;
  return (o0 + t) * d - (s - 1) + (h - t * e);
}

template <int KC>
__global__ __launch_bounds__(kRgThreads) void regrid_sample_kernel(const RegridSample S, const float *__restrict__ fin,
                                                                   float *__restrict__ fout) {
#pragma clang fp contract(off)
  extern __shared__ float rg_tile[];
  const int ox0 = blockIdx.x * kRgTX, oy0 = blockIdx.y * kRgTY, ok0 = blockIdx.z * KC;
  const int n = S.hx * S.hy * S.hk;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int hk = i % S.hk, hy = (i / S.hk) % S.hy, hx = i / (S.hk * S.hy);
    int ix2 = regrid_src(hx, S.ex, kRgTX, ox0, S.dx, S.sx);
    const int iy2 = regrid_src(hy, S.ey, kRgTY, oy0, S.dy, S.sy), ip2 = regrid_src(hk, S.ep, KC, ok0, S.dp, S.sp);
    if (ix2 < 0)
      ix2 += S.nx;
    else if (ix2 >= S.nx)
      ix2 -= S.nx;
    const bool inside = ix2 >= 0 && ix2 < S.nx && iy2 >= 0 && iy2 < S.ny && ip2 >= 0 && ip2 < S.np;
    rg_tile[i] = inside ? fin[((size_t) ix2 * S.ny + iy2) * (size_t) S.np + ip2] : 0.f;   // (outside: never summed)
  }
  __syncthreads();
  const int k = threadIdx.x % KC, ok = ok0 + k;
  const float fsx = (float) S.sx, fsy = (float) S.sy, fsp = (float) S.sp;
  const bool copy = S.sx == 1 && S.sy == 1 && S.sp == 1;
  for (int c = threadIdx.x / KC; c < kRgTX * kRgTY; c += blockDim.x / KC) {
    const int tx = c / kRgTY, ty = c % kRgTY, ox = ox0 + tx, oy = oy0 + ty;
    if (ox >= S.nx2 || oy >= S.ny2 || ok >= S.np2)
      continue;
    const int bx = tx * S.ex, by = ty * S.ey, bk = k * S.ep;
    const size_t to = ((size_t) ox * S.ny2 + oy) * (size_t) S.np2 + ok;
    if (copy) {
      fout[to] = rg_tile[(bx * S.hy + by) * S.hk + bk];
      continue;
    }
    // window entries of the clamped loop bounds (entry 0 is index i - s + 1)
    const int iy = oy * S.dy, ip = ok * S.dp;
    const int y_lo = iy - S.sy + 1 < 0 ? -(iy - S.sy + 1) : 0;
    const int y_hi = iy + S.sy - 1 > S.ny - 1 ? 2 * S.sy - 2 - (iy + S.sy - 1 - (S.ny - 1)) : 2 * S.sy - 2;
    const int p_lo = ip - S.sp + 1 < 0 ? -(ip - S.sp + 1) : 0;
    const int p_hi = ip + S.sp - 1 > S.np - 1 ? 2 * S.sp - 2 - (ip + S.sp - 1 - (S.np - 1)) : 2 * S.sp - 2;
    float a = 0.f, ws = 0.f;
    for (int ax = 0; ax < 2 * S.sx - 1; ax++) {
      const float wx = 1.0f - (float) abs(ax - (S.sx - 1)) / fsx;
      for (int ay = y_lo; ay <= y_hi; ay++) {
        const float wxy = wx * (1.0f - (float) abs(ay - (S.sy - 1)) / fsy);
        const float *row = rg_tile + ((bx + ax) * S.hy + (by + ay)) * S.hk + bk;
        for (int ap = p_lo; ap <= p_hi; ap++) {
          const float w = wxy * (1.0f - (float) abs(ap - (S.sp - 1)) / fsp);
          const float prod = w * row[ap];
          a = a + prod;
          ws = ws + w;
        }
      }
    }
    fout[to] = a / ws;
  }
}

}   // namespace mphip
