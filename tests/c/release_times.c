/* Test program (tests/test_backward_cpu.py): start / stop time of a run from the release times of its particles.
 * argv[1], argv[2] = earliest and latest release time (three particles: both and their mean), then control keys as on
 * trac's command line (DIRECTION, DT_MOD, T_STOP).  Prints: t_start t_stop */
#include "mptrac.h"

int main(int argc, char *argv[]) {
  ctl_t *ctl;
  cache_t *cache;
  clim_t *clim;
  met_t *met0, *met1;
  atm_t *atm;
  depo_t *depo;
  dd_t *dd;
  if (argc < 3)
    return 2;
  mptrac_alloc(&ctl, &cache, &clim, &met0, &met1, &atm, &depo, &dd);
  mptrac_read_ctl("-", argc, argv, ctl);
  const double first = atof(argv[1]), last = atof(argv[2]);
  atm->np = 3;
  atm->time[0] = 0.5 * (first + last);
  atm->time[1] = last;
  atm->time[2] = first;
  module_timesteps_init(ctl, atm);
  printf("RESULT %.17g %.17g\n", ctl->t_start, ctl->t_stop);
  return 0;
}
