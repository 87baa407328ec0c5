/* batch_driver.c -- a caller of solveCGBatch written ONLY against the reference-shaped API
 * (include/sparsebench/sparsebench.h): the set-up sequence of src/main.c:164-225 for a generated matrix, then nrhs CG solves
 * on one pass over the matrix per loop body.  Usage: batch_driver <n> <itermax> <eps> <nrhs>.  Built twice: -DCRS and -DSCS.
 */
#include <stdlib.h>

#include "sparsebench/sparsebench.h"

int main(int argc, char** argv)
{
  if (argc < 5) {
    fprintf(stderr, "usage: %s <n> <itermax> <eps> <nrhs>\n", argv[0]);
    return 2;
  }
  Comm comm;
  Parameter param;
  commInit(&comm, argc, argv);
  initParameter(&param);
  param.nx = param.ny = param.nz = atoi(argv[1]);
  param.itermax = atoi(argv[2]);
  param.eps     = atof(argv[3]);
  GMatrix m;
  matrixGenerate(&m, &param, comm.rank, comm.size, false);
  commPartition(&comm, &m);
  Matrix sm;
  memset(&sm, 0, sizeof sm);
#ifdef SCS
  sm.C = 64, sm.sigma = 1;
#endif
  convertMatrix(&sm, &m);
  size_t ff[NUMREGIONS] = { 0 }, fw[NUMREGIONS] = { 0 };
  ff[DDOT] = ff[WAXPBY] = m.totalNr, fw[DDOT] = fw[WAXPBY] = sizeof(CG_FLOAT) * (size_t)m.totalNr;
  ff[SPMVM] = m.totalNnz, fw[SPMVM] = 12 * (size_t)m.totalNnz;
  profilerInit(ff, fw);
  int k = solveCGBatch(&comm, &param, &sm, atoi(argv[4]));
  printf("k %d\n", k);
  profilerPrint(&comm, k);
  profilerFinalize();
  commFinalize(&comm);
  return EXIT_SUCCESS;
}
