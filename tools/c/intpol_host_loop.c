/* The host interpolation of write_grid, timed: mptrac_amd_intpol_3d (temperature) at the centres of an nx x ny x nz output
 * grid over the globe and 0 ... 30 km, one call per cell as write_grid makes them, from two MET_TYPE 1 files -- and then
 * from their MET_TYPE 2 conversions read with HIP_MET_PACKED 1, where the first call also decodes all level fields of both
 * snapshots on the device and downloads them (met_need_floats).  Two passes each: the second finds the floats in place.
 * tools/gpu_intpol_cost.py compiles this against a tree's host layer and reads the JSON line.
 *   intpol_host_loop <ctl> <met0.bin> <met1.bin> <scratch dir> <nx> <ny> <nz> [KEY VALUE ...] */
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "mptrac.h"

static double wall(void) {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double) ts.tv_sec + 1e-9 * (double) ts.tv_nsec;
}

static double loop(met_t *met0, met_t *met1, int nx, int ny, int nz, double t, double *sum) {
  const double t0 = wall();
  double s = 0;
  for (int i = 0; i < nx; i++)
    for (int j = 0; j < ny; j++)
      for (int k = 0; k < nz; k++) {
        const double lon = -180. + 360. / nx * (i + 0.5), lat = -90. + 180. / ny * (j + 0.5), z = 30. / nz * (k + 0.5);
        s += mptrac_amd_intpol_3d(met0, met1, offsetof(met_t, t), t, P(z), lon, lat);
      }
  *sum = s;
  return (wall() - t0) * 1e3;
}

int main(int argc, char *argv[]) {
  if (argc < 8)
    ERRMSG("Give parameters: <ctl> <met0> <met1> <scratch dir> <nx> <ny> <nz>");
  ctl_t *ctl;
  cache_t *cache;
  clim_t *clim;
  met_t *met0, *met1;
  atm_t *atm;
  mptrac_alloc(&ctl, &cache, &clim, &met0, &met1, &atm, NULL, NULL);
  mptrac_read_ctl(argv[1], argc, argv, ctl);
  const int nx = atoi(argv[5]), ny = atoi(argv[6]), nz = atoi(argv[7]);
  double ms[4], sum[4];
  ctl->met_type = 1;
  if (!mptrac_read_met(argv[2], ctl, clim, met0, NULL) || !mptrac_read_met(argv[3], ctl, clim, met1, NULL))
    ERRMSG("Cannot open file!");
  const double t = 0.5 * (met0->time + met1->time);
  ms[0] = loop(met0, met1, nx, ny, nz, t, &sum[0]);
  ms[1] = loop(met0, met1, nx, ny, nz, t, &sum[1]);
  char pck[2][LEN];
  ctl->met_type = 2;
  ctl->hip_met_packed = 1;
  for (int k = 0; k < 2; k++) {
    sprintf(pck[k], "%s/intpol_host_loop_%d.pck", argv[4], k);
    mptrac_write_met(pck[k], ctl, k ? met1 : met0);
  }
  if (!mptrac_read_met(pck[0], ctl, clim, met0, NULL) || !mptrac_read_met(pck[1], ctl, clim, met1, NULL))
    ERRMSG("Cannot open file!");
  ms[2] = loop(met0, met1, nx, ny, nz, t, &sum[2]);
  ms[3] = loop(met0, met1, nx, ny, nz, t, &sum[3]);
  remove(pck[0]);
  remove(pck[1]);
  printf("JSON {\"points\": %ld, \"float_files_ms\": [%.3f, %.3f], \"packed_files_ms\": [%.3f, %.3f], "
         "\"checksum_float\": %.17g, \"checksum_packed\": %.17g}\n", (long) nx * ny * nz, ms[0], ms[1], ms[2], ms[3], sum[0],
         sum[2]);
  return sum[0] == sum[1] && sum[2] == sum[3] ? EXIT_SUCCESS : EXIT_FAILURE;
}
