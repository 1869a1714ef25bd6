// mphip_ingest.hpp -- the kernels behind mphip_ingest_met: what lies between a netCDF file's values and a met_t.
//
// The definitions are transcribed from the host loops of read_met_nc (mptrac_amd/host/mptrac.c: nc_field, the lnsp
// conversion, the extrapolation loop, met_polar_winds / pole_row_from_neighbour, met_periodic); they are written out in
// include/mptrac_hip.h, at mphip_ingest_met, and restated independently in tests/refingest.py.  Every operation is the
// IEEE operation on the named type, rounded once and never contracted, in both builds, so both libraries return the
// host loops' bits.
//
// Layout.  A file holds a level field as [level][y][x], a met_t as [x][y][level]: the decode reverses the three axes.
// For a fixed y that is the transposition of an (x, level) plane, and a workgroup takes a kIgTile x kIgTile tile of it
// through LDS: global reads run along x (the file's fastest axis), global writes along the level (the met_t's), both
// coalesced; the tile is staged at the odd row pitch kIgTile + 1 (the convention of mphip_metprep.hpp), so the lanes of a
// wave touch 64 different banks in both passes.  The short decode and the mask happen between the load and the LDS store.
// Ragged edges are handled in the tile: a lane outside the extents loads and stores nothing.  A surface field is the same
// kernel with ny = 1 and its y axis in the place of the level.  The arrays on the device are compact, [nx2][ny][nlev]
// with the periodic column (if any) as the last one, so that column is one contiguous run.
#pragma once

#include "mphip_device.hpp"

namespace mphip {

constexpr int kIgTile = 64;                      // tile edge in x and in the level: one wave's width
constexpr int kIgThreads = 256;                  // four waves: each takes every fourth row of the tile
constexpr int kIgPitch = kIgTile + 1;            // odd pitch of the staged tile [x][level]
constexpr int kIgRows = kIgThreads / kIgTile;
constexpr int kIgFields = 11;                    // the level fields the extrapolation fills: t u v w h2o o3 lwc rwc iwc swc cc
constexpr int kIgMaxCopy = MPHIP_N3D + MPHIP_N2D;

// how the stored values of one field become floats (mphip_raw_t without its pointer)
struct IngestRaw {
  float scale_factor, add_offset;
  float fill_f, miss_f;      // MPHIP_RAW_FLOAT: compared as floats
  int fill_s, miss_s;        // MPHIP_RAW_SHORT: compared as the stored shorts
  float scl;
  int lnsp;
};

__device__ __forceinline__ float ig_nan() {
  return __uint_as_float(0x7fc00000u);
}

// keep ? scl v : NaN, and the surface pressure from its logarithm
__device__ __forceinline__ float ig_finish(float v, bool keep, const IngestRaw &R) {
#pragma clang fp contract(off)
  float r = keep ? R.scl * v : ig_nan();
  if (R.lnsp) {
    const double e = libm_exp((double) r);
    r = (float) (e / 100.);
  }
  return r;
}

__device__ __forceinline__ float ig_value(short raw, const IngestRaw &R) {
#pragma clang fp contract(off)
  const float prod = (float) raw * R.scale_factor;
  const float v = prod + R.add_offset;
  const bool keep = (R.fill_s == 0 || raw != R.fill_s) && (R.miss_s == 0 || raw != R.miss_s) && fabsf(v) < 1e14f;
  return ig_finish(v, keep, R);
}

__device__ __forceinline__ float ig_value(float v, const IngestRaw &R) {
  const bool keep = (R.fill_f == 0 || v != R.fill_f) && (R.miss_f == 0 || v != R.miss_f) && fabsf(v) < 1e14f;
  return ig_finish(v, keep, R);
}

// ---- decode + axis reversal: raw[k][j][i] -> out[i][j][k] -----------------------------------------------------------
// grid (ceil(nx / kIgTile), ny, ceil(nlev / kIgTile)); nx ny nlev < 2^31 (the caller refuses more)
template <typename T>
__global__ __launch_bounds__(kIgThreads) void ingest_decode_kernel(const T *__restrict__ raw, float *__restrict__ out, int nx,
                                                                   int ny, int nlev, IngestRaw R) {
  __shared__ float tile[kIgTile * kIgPitch];
  const int x0 = blockIdx.x * kIgTile, j = blockIdx.y, k0 = blockIdx.z * kIgTile;
  const int lane = threadIdx.x % kIgTile, row = threadIdx.x / kIgTile;
  if (x0 + lane < nx)
    for (int kk = row; kk < kIgTile && k0 + kk < nlev; kk += kIgRows) {
      const size_t at = ((size_t) (k0 + kk) * (size_t) ny + (size_t) j) * (size_t) nx + (size_t) (x0 + lane);
      tile[lane * kIgPitch + kk] = ig_value(raw[at], R);
    }
  __syncthreads();
  if (k0 + lane < nlev)
    for (int xx = row; xx < kIgTile && x0 + xx < nx; xx += kIgRows) {
      const size_t at = ((size_t) (x0 + xx) * (size_t) ny + (size_t) j) * (size_t) nlev + (size_t) (k0 + lane);
      out[at] = tile[xx * kIgPitch + lane];
    }
}

// ---- extrapolation below the lowest valid level ---------------------------------------------------------------------
// A wave per column, lanes over levels.  `low`, the largest level at which t, u, v or w is not finite, comes from ballots
// over chunks of 64 levels from the top down; then every field's levels 0 ... low take the bits of level low + 1 (0.f when
// there is none), all lanes at once.  The first four pointers are t, u, v, w; NULL: the field is absent (and counts as
// finite).
struct IngestColumns {
  float *f[kIgFields];
};

__global__ __launch_bounds__(kIgThreads) void ingest_extrapolate_kernel(IngestColumns F, int ncol, int np) {
  const int lane = threadIdx.x % 64;
  const long long col = (long long) blockIdx.x * (kIgThreads / 64) + threadIdx.x / 64;
  if (col >= ncol)
    return;
  const size_t base = (size_t) col * (size_t) np;
  int low = -1;
  for (int c0 = ((np - 1) / 64) * 64; c0 >= 0; c0 -= 64) {
    const int k = c0 + lane;
    bool bad = false;
    if (k < np)
#pragma unroll
      for (int f = 0; f < 4; f++)
        if (F.f[f])
          bad |= !(fabsf(F.f[f][base + k]) < __builtin_inff());
    const unsigned long long m = __ballot(bad);
    if (m) {
      low = c0 + 63 - __clzll((long long) m);
      break;
    }
  }
  if (low < 0)
    return;
#pragma unroll
  for (int f = 0; f < kIgFields; f++)
    if (F.f[f]) {
      float *const col_f = F.f[f] + base;
      const float v = low + 1 < np ? col_f[low + 1] : 0.f;
      for (int k = lane; k <= low; k += 64)
        col_f[k] = v;
    }
}

// ---- pole rows of u, v from their neighbour rows --------------------------------------------------------------------
// A lane per level of one pole, serial over the longitudes in their order (the order of the sum is the definition); the
// lanes of a wave read consecutive levels.  c, s: the nx cosines and sines of the pole's frame, built on the host.  nx is
// the extent without the periodic column.
__global__ __launch_bounds__(64) void ingest_polar_kernel(float *__restrict__ u, float *__restrict__ v, int nx, int ny, int np,
                                                          int pole, int next, const double *__restrict__ c,
                                                          const double *__restrict__ s) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= np)
    return;
  const double n = (double) nx;
  double mx = 0, my = 0;
  for (int ix = 0; ix < nx; ix++) {
    const size_t at = ((size_t) ix * (size_t) ny + (size_t) next) * (size_t) np + (size_t) k;
    const double uu = u[at], vv = v[at], cc = c[ix], ss = s[ix];
    const double uc = uu * cc, vs = vv * ss, us = uu * ss, vc = vv * cc;
    const double dx = uc - vs, dy = us + vc;
    const double qx = dx / n, qy = dy / n;
    mx = mx + qx;
    my = my + qy;
  }
  for (int ix = 0; ix < nx; ix++) {
    const size_t at = ((size_t) ix * (size_t) ny + (size_t) pole) * (size_t) np + (size_t) k;
    const double cc = c[ix], ss = s[ix];
    const double a = mx * cc, b = my * ss, d = my * cc, e = mx * ss;
    const double un = a + b, vn = d - e;
    u[at] = (float) un;
    v[at] = (float) vn;
  }
}

// ---- the periodic column: column nx of every field is a copy of column 0 ------------------------------------------------
// one launch for all fields (grid.y = the field): n[f] = ny nlev values from p[f] to p[f] + nx n[f]
struct IngestCopy {
  float *p[kIgMaxCopy];
  unsigned n[kIgMaxCopy];
};

__global__ __launch_bounds__(kIgThreads) void ingest_periodic_kernel(IngestCopy C, int nx) {
  float *const p = C.p[blockIdx.y];
  const unsigned n = C.n[blockIdx.y];
  float *const dst = p + (size_t) nx * (size_t) n;
  for (unsigned i = blockIdx.x * kIgThreads + threadIdx.x; i < n; i += gridDim.x * kIgThreads)
    dst[i] = p[i];
}

}   // namespace mphip
