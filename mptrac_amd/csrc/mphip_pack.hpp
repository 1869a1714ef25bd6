// mphip_pack.hpp -- the 16-bit packed level fields of MET_TYPE 2 files: the decoder behind mphip_update_met_packed,
// mphip_prefetch_met_packed and mphip_unpack_met, and the encoder behind mphip_pack_met.
//
// The definition is this project's own statement (include/mptrac_hip.h, at mphip_met_packed_t; restated independently in
// tests/refpack.py): one scale and one offset per level, double arithmetic that is never contracted, a true division in
// the encoder in both builds -- so both libraries return the restatement's bits.
//
// Layout.  A level field is [ix][iy][ip] with ip fastest, codes and floats alike, so both streaming kernels see one run
// of n = nx ny nlev values whose level is the index modulo nlev.  A lane owns 8 consecutive values: 16 bytes of codes
// (one dwordx4) against 32 bytes of floats (two dwordx4).  The level of a lane's first value costs one integer division;
// its seven neighbours and the lane's next run (a grid stride further) follow by an add and a compare-and-wrap.  scl / off
// are read from a table in LDS, {scl, off} pairs that every workgroup copies once, while 16 nlev bytes fit 64 KB
// (kPkLdsLevels), and from global memory above.  The vector path starts at the first code that is 16-byte aligned
// (`head` values in) and block 0 does those and the n mod 8 values at the end one by one.  The floats behind an odd head
// are only 4-byte aligned: their vector type says so.
#pragma once

#include "mphip_device.hpp"

namespace mphip {

constexpr int kPkThreads = 256;
constexpr int kPkVec = 8;                       // values per lane and pass
constexpr int kPkMaxBlocks = 2048;              // 256 CUs x 8 workgroups; the rest is a grid stride
constexpr int kPkLdsLevels = 64 * 1024 / 16;    // most levels whose {scl, off} table fits the LDS of a workgroup
constexpr int kPkRedLevels = 64;                // levels per workgroup of the reduction of the partial extremes
constexpr int kPkRedThreads = 1024;             // ... whose 16 waves each take every 16th workgroup's partials

typedef unsigned short pk_codes __attribute__((ext_vector_type(8)));                 // 16 bytes, aligned
typedef float pk_floats __attribute__((ext_vector_type(4), aligned(4)));             // 16 bytes at any float

// v = (float) ((double) q scl + off), then the reader's limits: fminf(fmaxf(v, lo), hi) as the C library evaluates them
// (the first argument unless the comparison says otherwise: a NaN becomes lo, a zero keeps its sign)
__device__ __forceinline__ float pk_decode(unsigned q, double scl, double off, float lo, float hi) {
#pragma clang fp contract(off)
  const double prod = (double) q * scl;
  const double sum = prod + off;
  float v = (float) sum;
  v = v >= lo ? v : lo;
  v = v <= hi ? v : hi;
  return v;
}

// q = (unsigned short) (((double) x - off) / scl + .5): an IEEE division in both builds
__device__ __forceinline__ unsigned short pk_encode(float x, double scl, double off) {
#pragma clang fp contract(off)
  const double d = (double) x - off;
  const double r = d / scl;
  const double h = r + .5;
  return (unsigned short) h;
}

// {scl, off} of a level: from the workgroup's table or from global memory
template <bool LDS>
struct PkTable {
  const double *tab, *scl, *off;
  __device__ __forceinline__ void init(double *smem, const double *__restrict__ s, const double *__restrict__ o, unsigned nlev) {
    scl = s;
    off = o;
    tab = smem;
    if (LDS) {
      for (unsigned k = threadIdx.x; k < nlev; k += kPkThreads) {
        smem[2 * k] = s[k];
        smem[2 * k + 1] = o[k];
      }
      __syncthreads();
    }
  }
  __device__ __forceinline__ void at(unsigned lev, double &s, double &o) const {
    if (LDS) {
      s = tab[2 * lev];
      o = tab[2 * lev + 1];
    } else {
      s = scl[lev];
      o = off[lev];
    }
  }
};

// the values block 0 does one by one: [0, head) and [body_end, n)
__device__ __forceinline__ unsigned pk_tail_index(unsigned t, unsigned head, unsigned body_end) {
  return t < head ? t : body_end + (t - head);
}

// ---- codes -> floats ------------------------------------------------------------------------------------------------
// n < 2^31 values (the callers refuse more), head <= n, (q + head) 16-byte aligned or n - head < 8
template <bool LDS>
__global__ __launch_bounds__(kPkThreads) void met_unpack_kernel(const unsigned short *__restrict__ q,
                                                                const double *__restrict__ scl, const double *__restrict__ off,
                                                                float *__restrict__ out, unsigned n, unsigned nlev, unsigned head,
                                                                float lo, float hi) {
  extern __shared__ double pk_smem[];
  PkTable<LDS> T;
  T.init(pk_smem, scl, off, nlev);
  const unsigned nvec = (n - head) / kPkVec, stride = gridDim.x * kPkThreads;
  unsigned g = blockIdx.x * kPkThreads + threadIdx.x;
  if (g < nvec) {
    unsigned lev = (head + g * kPkVec) % nlev;
    const unsigned step = (unsigned) (((unsigned long long) stride * kPkVec) % nlev);     // (the same in every lane)
    for (; g < nvec; g += stride) {
      const size_t i = head + (size_t) g * kPkVec;
      const pk_codes c = *(const pk_codes *) (q + i);
      float v[kPkVec];
      unsigned l = lev;
#pragma unroll
      for (int j = 0; j < kPkVec; j++) {
        double s, o;
        T.at(l, s, o);
        v[j] = pk_decode(c[j], s, o, lo, hi);
        l = l + 1 == nlev ? 0 : l + 1;
      }
      pk_floats a = { v[0], v[1], v[2], v[3] }, b = { v[4], v[5], v[6], v[7] };
      *(pk_floats *) (out + i) = a;
      *(pk_floats *) (out + i + 4) = b;
      lev += step;
      if (lev >= nlev)
        lev -= nlev;
    }
  }
  if (blockIdx.x == 0) {
    const unsigned body_end = head + nvec * kPkVec, ntail = head + (n - body_end);
    for (unsigned t = threadIdx.x; t < ntail; t += kPkThreads) {
      const unsigned i = pk_tail_index(t, head, body_end);
      double s, o;
      T.at(i % nlev, s, o);
      out[i] = pk_decode(q[i], s, o, lo, hi);
    }
  }
}

// ---- floats -> codes: the mirror ------------------------------------------------------------------------------------
// (q + head) 16-byte aligned or n - head < 8; x is only float-aligned behind an odd head
template <bool LDS>
__global__ __launch_bounds__(kPkThreads) void met_pack_quantise_kernel(const float *__restrict__ x, const double *__restrict__ scl,
                                                                       const double *__restrict__ off,
                                                                       unsigned short *__restrict__ q, unsigned n, unsigned nlev,
                                                                       unsigned head) {
  extern __shared__ double pk_smem[];
  PkTable<LDS> T;
  T.init(pk_smem, scl, off, nlev);
  const unsigned nvec = (n - head) / kPkVec, stride = gridDim.x * kPkThreads;
  unsigned g = blockIdx.x * kPkThreads + threadIdx.x;
  if (g < nvec) {
    unsigned lev = (head + g * kPkVec) % nlev;
    const unsigned step = (unsigned) (((unsigned long long) stride * kPkVec) % nlev);
    for (; g < nvec; g += stride) {
      const size_t i = head + (size_t) g * kPkVec;
      const pk_floats a = *(const pk_floats *) (x + i), b = *(const pk_floats *) (x + i + 4);
      const float v[kPkVec] = { a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3] };
      pk_codes c;
      unsigned l = lev;
#pragma unroll
      for (int j = 0; j < kPkVec; j++) {
        double s, o;
        T.at(l, s, o);
        c[j] = pk_encode(v[j], s, o);
        l = l + 1 == nlev ? 0 : l + 1;
      }
      *(pk_codes *) (q + i) = c;
      lev += step;
      if (lev >= nlev)
        lev -= nlev;
    }
  }
  if (blockIdx.x == 0) {
    const unsigned body_end = head + nvec * kPkVec, ntail = head + (n - body_end);
    for (unsigned t = threadIdx.x; t < ntail; t += kPkThreads) {
      const unsigned i = pk_tail_index(t, head, body_end);
      double s, o;
      T.at(i % nlev, s, o);
      q[i] = pk_encode(x[i], s, o);
    }
  }
}

// ---- per-level extremes ---------------------------------------------------------------------------------------------
// A workgroup stages its run of cpb consecutive columns -- they are contiguous -- in LDS with coalesced loads, at the odd
// pitch nlev | 1 of mphip_metprep.hpp, and a lane per level then walks the staged columns: one partial {min, max, a value
// that is not finite was seen} per workgroup and level, [workgroup][level].  Minimum and maximum do not depend on the
// order they are taken in (a zero's sign would: the reduction below gives off the sign +), so the partials are reduced by
// a second launch in any order and without atomics.
__global__ __launch_bounds__(kPkThreads) void met_pack_extremes_kernel(const float *__restrict__ x, int ncol, int nlev, int cpb,
                                                                       int pitch, float *__restrict__ pmin,
                                                                       float *__restrict__ pmax, int *__restrict__ pbad) {
  extern __shared__ float pk_plane[];
  const int col0 = blockIdx.x * cpb, left = ncol - col0, ncols = left < cpb ? left : cpb;
  const int nval = ncols * nlev;
  const float *__restrict__ src = x + (size_t) col0 * (size_t) nlev;
  for (int i = threadIdx.x; i < nval; i += kPkThreads) {
    const int c = i / nlev, k = i - c * nlev;
    pk_plane[c * pitch + k] = src[i];
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nlev; k += kPkThreads) {
    float lo = __builtin_inff(), hi = -__builtin_inff();
    int bad = 0;
    for (int c = 0; c < ncols; c++) {
      const float v = pk_plane[c * pitch + k];
      bad |= !(fabsf(v) < __builtin_inff());
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    }
    const size_t at = (size_t) blockIdx.x * (size_t) nlev + k;
    pmin[at] = lo;
    pmax[at] = hi;
    pbad[at] = bad;
  }
}

// the partials of kPkRedLevels levels per workgroup, kPkRedThreads / kPkRedLevels slices of them side by side (the loop is
// bound by the latency of its loads: 4067 partials per level on the 721 x 361 grid), then off = min
// (+ 0.: a zero of either sign is stored as +0.) and scl = (max != min) ? (max - min) / 65533. : 1.
__global__ __launch_bounds__(kPkRedThreads) void met_pack_reduce_kernel(const float *__restrict__ pmin, const float *__restrict__ pmax,
                                                                     const int *__restrict__ pbad, int nblk, int nlev,
                                                                     double *__restrict__ scl, double *__restrict__ off,
                                                                     int *__restrict__ bad) {
#pragma clang fp contract(off)
  __shared__ float slo[kPkRedThreads], shi[kPkRedThreads];
  __shared__ int sbad[kPkRedThreads];
  constexpr int kParts = kPkRedThreads / kPkRedLevels;
  const int part = threadIdx.x / kPkRedLevels, k = blockIdx.x * kPkRedLevels + threadIdx.x % kPkRedLevels;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  int b = 0;
  if (k < nlev)
    for (int blk = part; blk < nblk; blk += kParts) {
      const size_t at = (size_t) blk * (size_t) nlev + k;
      const float l = pmin[at], h = pmax[at];
      lo = l < lo ? l : lo;
      hi = h > hi ? h : hi;
      b |= pbad[at];
    }
  slo[threadIdx.x] = lo;
  shi[threadIdx.x] = hi;
  sbad[threadIdx.x] = b;
  __syncthreads();
  if (part == 0 && k < nlev) {
    for (int p = 1; p < kParts; p++) {
      const float l = slo[threadIdx.x + p * kPkRedLevels], h = shi[threadIdx.x + p * kPkRedLevels];
      lo = l < lo ? l : lo;
      hi = h > hi ? h : hi;
      b |= sbad[threadIdx.x + p * kPkRedLevels];
    }
    const double mn = (double) lo + 0., mx = (double) hi;
    const double range = mx - mn;
    off[k] = mn;
    scl[k] = mx != mn ? range / 65533. : 1.;
    bad[k] = b;
  }
}

}   // namespace mphip
