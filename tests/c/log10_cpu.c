/* log10_cpu.c -- test infrastructure: mphip_libm_log10 of mptrac_amd/csrc/mphip_libm.h (the device's log10, glibc's
 * __ieee754_log10 on top of the restated log) compiled for the CPU and compared bit by bit with the running C
 * library's log10.  Built by tests/test_oh_chem_host.py (gcc -O2 -ffp-contract=off [-mfma]). */
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
  return ua == ub || (a != a && b != b);     /* any NaN equals any NaN */
}

/* number of arguments whose restated value differs from the library's; first_bad = index of the first one */
size_t cmp_log10(const double *x, size_t n, size_t *first_bad) {
  size_t bad = 0;
#pragma omp parallel for schedule(static) reduction(+ : bad)
  for (size_t i = 0; i < n; i++)
    if (!same(mphip_libm_log10(mphip_libm_log_tab, x[i]), log10(x[i]))) {
      bad++;
#pragma omp critical
      if (i < *first_bad)
        *first_bad = i;
    }
  return bad;
}
