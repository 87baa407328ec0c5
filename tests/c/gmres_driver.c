/* gmres_driver.c -- a caller of solveGMRES written ONLY against the reference-shaped API
 * (include/sparsebench/sparsebench.h): the set-up sequence of src/main.c:164-225, then the solver the reference's driver
 * names and leaves empty.  Usage: gmres_driver <file.mtx> <itermax> <eps> <restart>.  Built twice: -DCRS and -DSCS.
 */
#include <stdlib.h>

#include "sparsebench/sparsebench.h"

int main(int argc, char** argv)
{
  if (argc < 5) {
    fprintf(stderr, "usage: %s <file.mtx> <itermax> <eps> <restart>\n", argv[0]);
    return 2;
  }
  Comm comm;
  Parameter param;
  commInit(&comm, argc, argv);
  initParameter(&param);
  param.filename = argv[1];
  param.itermax  = atoi(argv[2]);
  param.eps      = atof(argv[3]);
  MMMatrix mm, local;
  GMatrix m;
  memset(&mm, 0, sizeof mm), memset(&local, 0, sizeof local);
  MMMatrixRead(&mm, param.filename);
  commDistributeMatrix(&comm, &mm, &local);
  matrixConvertfromMM(&local, &m);
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
  int k = solveGMRES(&comm, &param, &sm, atoi(argv[4]));
  printf("k %d\n", k);
  profilerPrint(&comm, k);
  profilerFinalize();
  commFinalize(&comm);
  return EXIT_SUCCESS;
}
