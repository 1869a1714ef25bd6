/* libm_wide_cpu.c -- test infrastructure: mphip_libm_cos_wide / mphip_libm_sin_wide of mptrac_amd/csrc/mphip_libm.h
 * (the cos / sin of geo2cart's longitudes on the device) compiled for the CPU and compared bit by bit with the running
 * C library's cos / sin.  Built by tests/test_libm_sincos_wide.py (gcc -O2 -ffp-contract=off -mfma).
 * With -DLIBM_WIDE_UNFUSED every fused multiply-add of the header becomes a multiplication and an addition, rounded
 * one after the other: a restatement that is NOT the library's, which the comparison has to find. */
#ifdef LIBM_WIDE_UNFUSED
#define __builtin_fma(a, b, c) ((a) * (b) + (c))
#endif
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "mphip_libm.h"
#include "mphip_libmtab.h"

static int same(double a, double b) {
  uint64_t ua, ub;
  memcpy(&ua, &a, 8);
  memcpy(&ub, &b, 8);
  return ua == ub || (a != a && b != b);
}

/* which: 0 cos, 1 sin.  Number of arguments that are not handled or whose value differs from the library's. */
size_t cmp_wide(int which, const double *x, size_t n, size_t *first_bad) {
  size_t bad = 0;
#pragma omp parallel for schedule(static) reduction(+ : bad)
  for (size_t i = 0; i < n; i++) {
    int handled;
    const double v = which ? mphip_libm_sin_wide(mphip_libm_sincos_tab, x[i], &handled)
                           : mphip_libm_cos_wide(mphip_libm_sincos_tab, x[i], &handled);
    if (!handled || !same(v, which ? sin(x[i]) : cos(x[i]))) {
      bad++;
#pragma omp critical
      if (i < *first_bad)
        *first_bad = i;
    }
  }
  return bad;
}

void rst_wide(int which, const double *x, size_t n, double *out, int *handled) {
  for (size_t i = 0; i < n; i++)
    out[i] = which ? mphip_libm_sin_wide(mphip_libm_sincos_tab, x[i], &handled[i])
                   : mphip_libm_cos_wide(mphip_libm_sincos_tab, x[i], &handled[i]);
}

/* the reduction constants the header carries as literals against the generated table header */
int check_wide_constants(void) {
  const double k[6] = { MPHIP_SC_HPINV, MPHIP_SC_TOINT, MPHIP_SC_MP1, MPHIP_SC_MP2, MPHIP_SC_PP3, MPHIP_SC_PP4 };
  for (int i = 0; i < 6; i++)
    if (k[i] != mphip_libm_sincos_k[14 + i])
      return 1 + i;
  return 0;
}
