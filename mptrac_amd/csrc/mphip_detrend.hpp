// mphip_detrend.hpp -- the last kernel-worthy step of the reference's meteo preprocessing: detrending
// (read_met_detrend), the kernel behind mphip_detrend_met.  A Gaussian-weighted horizontal mean (the background) is
// subtracted from t, u, v and w.
//
// The definition is this project's own statement (include/mptrac_hip.h, at mphip_detrend_met; restated independently in
// tests/refdetrend.py).  The weights come from the host as one table per call (double arithmetic and the C library's
// exp / cos / sin, each weight rounded to float once); the stencil is float arithmetic in a fixed order, never contracted.
//
// Layout.  The fields are [ix][iy][ip] with ip fastest, as in mphip_metprep.hpp.
//   A workgroup owns one latitude row iy of one field.  Its weights w(iy, iy2, d) depend on the row pair and on the
// longitude offset d = |ix - ix2| only, so every lane of the workgroup multiplies by the same weight: the table is read
// through the scalar cache and the weight is an SGPR operand of the multiply -- no exp in the stencil, no weight in LDS
// or in a VGPR.  The window is (2 sx + 1) x (2 sy + 1) with sx up to nx / 2 next to the poles (the table of one row is up
// to 131 KB on the 721 x 361 grid), so nothing is staged with a fixed halo: the inputs are read from L2 / L1 as runs of
// consecutive levels, and what cuts the loads is register blocking -- a lane owns kDtTX consecutive longitudes of one
// level and walks the columns ix0 - sx ... ix0 + kDtTX - 1 + sx once; a value it loads enters up to kDtTX sums, each
// with the weight of its own offset.  Per point the order of summation is the definition's: columns ascending (the outer
// loop over ix2), rows ascending inside.  The lanes of a row are the flattened (longitude group, level) pairs with the
// level fastest: a wave's loads stay runs of consecutive floats and level counts that are no multiple of 64 leave no
// idle lanes.  The weight sum ws does not depend on ix or ip: the host forms it per row by the same serial float
// additions in the same order.
#pragma once

#include "mphip_device.hpp"

namespace mphip {

constexpr int kDtFields = 4;           // t, u, v, w
constexpr int kDtThreads = 256;
constexpr int kDtTX = 8;               // longitudes per lane

struct DetrendRow {
  long long off;     // first weight of the row in the table: w[(iy2 - ylo) (sx + 1) + d]
  int sx;            // half-width along x, 1 ... nx / 2
  int ylo, nr;       // first row and number of rows of the window (clamped to the grid)
  float ws;          // the sum of the window's weights in the definition's order
};

struct __attribute__((aligned(4))) DetrendW {      // kDtTX consecutive weights of one table row: what one column needs
  float w[kDtTX];
};

struct DetrendFields {
  int n;
  const float *in[kDtFields];
  float *out[kDtFields];
};

// One column of the window: its nr values enter the sums b[jlo ... jhi] of the lane, row by row.  The kDtTX weights of a
// table row that the column needs are consecutive entries from wq on -- one scalar load of kDtTX floats per row and a
// running pointer, so that the scalar unit, which every wave of the CU shares, is not what the loop waits for --; which
// entry belongs to which sum is known at compile time: KIND 0 (the column lies at or left of the lane's first point, e
// <= 0): entry j; KIND 1 (at or right of its last point, e >= kDtTX - 1): entry kDtTX - 1 - j; KIND 2 (between, e = E):
// entry |E - j|.  Entries of sums outside jlo ... jhi may lie beyond the row (the table ends with kDtTX floats of
// padding): they are loaded and never used.
template <int KIND, int E>
__device__ __forceinline__ void detrend_column(float (&b)[kDtTX], const float *__restrict__ col, const float *__restrict__ wq,
                                               int nr, int np, int pitch, int jlo, int jhi) {
#pragma clang fp contract(off)
  if (jlo == 0 && jhi == kDtTX - 1) {
#pragma unroll 4                                // (four loads in flight per lane; the sums stay in order)
    for (int r = 0; r < nr; r++) {
      const float v = col[(size_t) r * np];
      const DetrendW wv = *(const DetrendW *) (wq + (size_t) r * pitch);
#pragma unroll
      for (int j = 0; j < kDtTX; j++) {
        const float prod = wv.w[KIND == 0 ? j : KIND == 1 ? kDtTX - 1 - j : (E > j ? E - j : j - E)] * v;
        b[j] = b[j] + prod;
      }
    }
  } else {
#pragma unroll 2
    for (int r = 0; r < nr; r++) {
      const float v = col[(size_t) r * np];
      const DetrendW wv = *(const DetrendW *) (wq + (size_t) r * pitch);
#pragma unroll
      for (int j = 0; j < kDtTX; j++)
        if (j >= jlo && j <= jhi) {
          const float prod = wv.w[KIND == 0 ? j : KIND == 1 ? kDtTX - 1 - j : (E > j ? E - j : j - E)] * v;
          b[j] = b[j] + prod;
        }
    }
  }
}

// grid: x = chunk * ny + iy, y = field.  The row is the fast index of the grid: the workgroups that run at the same time
// own the same longitudes of neighbouring rows and walk the same columns at about the same time, so what they read at any
// moment is a few columns (198 KB each on the 721 x 361 x 137 grid), which the L2 holds, and not the whole field
__global__ __launch_bounds__(kDtThreads) void detrend_kernel(int nx, int ny, int np,
                                                             const DetrendRow *__restrict__ rows,
                                                             const float *__restrict__ wt, const DetrendFields F) {
#pragma clang fp contract(off)
  static_assert(kDtTX == 8, "the dispatch below names the columns 1 ... kDtTX - 2");
  const int chunk = blockIdx.x / ny, iy = blockIdx.x - chunk * ny;
  const int ngroup = (nx + kDtTX - 1) / kDtTX;
  const long long lane = (long long) chunk * kDtThreads + threadIdx.x;
  if (lane >= (long long) ngroup * np)
    return;
  const int g = (int) (lane / np), ip = (int) (lane - (long long) g * np), ix0 = g * kDtTX;
  const DetrendRow R = rows[iy];
  const int sx = R.sx, pitch = sx + 1, nr = R.nr;
  const float *__restrict__ w0 = wt + R.off;
  const float *__restrict__ fin = F.in[blockIdx.y];
  const size_t colstride = (size_t) ny * np;
  float b[kDtTX];
#pragma unroll
  for (int j = 0; j < kDtTX; j++)
    b[j] = 0.f;
  for (int e = -sx; e <= kDtTX - 1 + sx; e++) {
    // the column: ix2 = ix0 + e wrapped once by +-nx.  A column that is still outside serves only the points ix0 + j >=
    // nx of the last group, which are not stored: any column will do for it
    int c = ix0 + e;
    if (c < 0)
      c += nx;
    else if (c >= nx)
      c -= nx;
    if (c < 0 || c >= nx)
      c = 0;
    const float *__restrict__ col = fin + (size_t) c * colstride + (size_t) R.ylo * np + ip;
    // the sums the column enters: |e - j| <= sx
    const int jlo = e - sx > 0 ? e - sx : 0, jhi = e + sx < kDtTX - 1 ? e + sx : kDtTX - 1;
    if (e <= 0)
      detrend_column<0, 0>(b, col, w0 + (-e), nr, np, pitch, jlo, jhi);                 // d = j - e
    else if (e >= kDtTX - 1)
      detrend_column<1, 0>(b, col, w0 + (e - (kDtTX - 1)), nr, np, pitch, jlo, jhi);    // d = e - j
    else
      switch (e) {                                                                      // d = |e - j|: entries 0 ... 7
      case 1: detrend_column<2, 1>(b, col, w0, nr, np, pitch, jlo, jhi); break;
      case 2: detrend_column<2, 2>(b, col, w0, nr, np, pitch, jlo, jhi); break;
      case 3: detrend_column<2, 3>(b, col, w0, nr, np, pitch, jlo, jhi); break;
      case 4: detrend_column<2, 4>(b, col, w0, nr, np, pitch, jlo, jhi); break;
      case 5: detrend_column<2, 5>(b, col, w0, nr, np, pitch, jlo, jhi); break;
      default: detrend_column<2, 6>(b, col, w0, nr, np, pitch, jlo, jhi); break;
      }
  }
  float *__restrict__ fout = F.out[blockIdx.y];
#pragma unroll
  for (int j = 0; j < kDtTX; j++)
    if (ix0 + j < nx) {
      const size_t at = ((size_t) (ix0 + j) * ny + iy) * (size_t) np + ip;
      fout[at] = fin[at] - b[j] / R.ws;
    }
}

}   // namespace mphip
