/* Test program (tests/test_ingest_cpu.py): a netCDF meteo file through the host layer's reader, on the host alone.
 *   ingest_host <file.nc> <dump> <coord_type>
 * reads <file.nc> with mptrac_read_met (MET_TYPE 0, HIP_MET_PREP 0, HIP_MET_INGEST 0: the host loops that are the
 * definition of mphip_ingest_met) into a fresh met_t and writes to <dump>: nx, ny, np as int32, lon[nx] as doubles, the
 * eleven level fields as compact floats [nx][ny][np] and the thirteen surface fields the reader fills as [nx][ny]. */
#include "mptrac.h"

int main(int argc, char *argv[]) {
  ctl_t *ctl;
  cache_t *cache;
  clim_t *clim;
  met_t *met, *spare;
  atm_t *atm;
  depo_t *depo;
  dd_t *dd;
  if (argc < 4)
    return 2;
  mptrac_alloc(&ctl, &cache, &clim, &met, &spare, &atm, &depo, &dd);
  char *keys[] = { argv[0], "-", "-", "-", "MET_TYPE", "0", "MET_COORD_TYPE", argv[3], "MET_UTM_REF_LAT", "50",
    "MET_UTM_REF_LON", "10", "MET_PBL", "0", "MET_CAPE", "0", "HIP_MET_PREP", "0", "HIP_MET_INGEST", "0" };
  mptrac_read_ctl("-", (int) (sizeof(keys) / sizeof(keys[0])), keys, ctl);
  memset(met, 0, sizeof(*met));
  if (!mptrac_read_met(argv[1], ctl, clim, met, dd))
    ERRMSG("Cannot read the file!");
  FILE *out = fopen(argv[2], "wb");
  if (!out)
    ERRMSG("Cannot create the dump!");
  const int dims[3] = { met->nx, met->ny, met->np };
  fwrite(dims, sizeof(int), 3, out);
  fwrite(met->lon, sizeof(double), (size_t) met->nx, out);
  float (*f3[])[EY][EP] = { met->t, met->u, met->v, met->w, met->h2o, met->o3, met->lwc, met->rwc, met->iwc, met->swc,
    met->cc };
  float (*f2[])[EY] = { met->ps, met->zs, met->ts, met->us, met->vs, met->ess, met->nss, met->shf, met->lsm, met->sst,
    met->pbl, met->cape, met->cin };
  for (size_t f = 0; f < sizeof(f3) / sizeof(f3[0]); f++)
    for (int i = 0; i < met->nx; i++)
      for (int j = 0; j < met->ny; j++)
        fwrite(f3[f][i][j], sizeof(float), (size_t) met->np, out);
  for (size_t f = 0; f < sizeof(f2) / sizeof(f2[0]); f++)
    for (int i = 0; i < met->nx; i++)
      fwrite(f2[f][i], sizeof(float), (size_t) met->ny, out);
  fclose(out);
  printf("RESULT %d %d %d\n", met->nx, met->ny, met->np);
  return 0;
}
