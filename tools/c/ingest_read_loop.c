/* mptrac_read_met of one netCDF file, timed, with HIP_MET_INGEST 0 (the reader's own loops) and 1 (mphip_ingest_met)
 * alternating in one process; the file is in the page cache after the first read.  tools/gpu_met_ingest_cost.py compiles
 * this against the tree's host layer with production extents and reads the JSON line.
 *   ingest_read_loop <ctl> <file.nc> <rounds> [KEY VALUE ...] */
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

int main(int argc, char *argv[]) {
  if (argc < 4)
    ERRMSG("Give parameters: <ctl> <file.nc> <rounds>");
  ctl_t *ctl;
  cache_t *cache;
  clim_t *clim;
  met_t *met0, *met1;
  atm_t *atm;
  mptrac_alloc(&ctl, &cache, &clim, &met0, &met1, &atm, NULL, NULL);
  mptrac_read_ctl(argv[1], argc, argv, ctl);
  const int rounds = atoi(argv[3]);
  double *ms[2];
  unsigned sum[2] = { 0, 0 };
  for (int on = 0; on < 2; on++)
    ms[on] = (double *) calloc((size_t) rounds + 1, sizeof(double));
  for (int r = 0; r <= rounds; r++)      /* (round 0: the warm-up -- page cache, device context, scratch pool) */
    for (int on = 0; on < 2; on++) {
      ctl->hip_met_ingest = on;
      met_t *met = on ? met1 : met0;
      const double t0 = wall();
      if (!mptrac_read_met(argv[2], ctl, clim, met, NULL))
        ERRMSG("Cannot open file!");
      ms[on][r] = (wall() - t0) * 1e3;
      printf("round %d HIP_MET_INGEST %d: %.1f ms\n", r, on, ms[on][r]);
      fflush(stdout);
    }
  /* the two snapshots are the same bytes */
  const size_t n3 = sizeof(met0->t) / sizeof(unsigned);
  const unsigned *a[] = { (unsigned *) met0->t, (unsigned *) met0->u, (unsigned *) met0->v, (unsigned *) met0->w, (unsigned *) met0->h2o },
    *b[] = { (unsigned *) met1->t, (unsigned *) met1->u, (unsigned *) met1->v, (unsigned *) met1->w, (unsigned *) met1->h2o };
  size_t differ = 0;
  for (int f = 0; f < 5; f++)
    for (size_t i = 0; i < n3; i++) {
      differ += a[f][i] != b[f][i];
      sum[0] += a[f][i];
      sum[1] += b[f][i];
    }
  printf("JSON {\"grid\": [%d, %d, %d], \"differ\": %zu, \"checksum\": [%u, %u], \"ms_ingest_0\": [", met0->nx, met0->ny, met0->np,
         differ, sum[0], sum[1]);
  for (int on = 0; on < 2; on++) {
    for (int r = 1; r <= rounds; r++)
      printf("%s%.3f", r > 1 ? ", " : "", ms[on][r]);
    printf(on ? "]}\n" : "], \"ms_ingest_1\": [");
  }
  return 0;
}
