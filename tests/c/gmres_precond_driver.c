/* gmres_precond_driver.c -- a caller of solveGMRESPrecond written ONLY against the reference-shaped API
 * (include/sparsebench/sparsebench.h): the set-up sequence of src/main.c:164-225 for a generated matrix or a Matrix Market file,
 * then GMRES(restart) right-preconditioned by one of PCG's preconditioners at its defaults.
 * Usage: gmres_precond_driver <n | file.mtx> <itermax> <eps> <restart> <precond>: a first argument that starts with a digit
 * generates the n^3 grid, any other is read as a Matrix Market file; precond: 0 jacobi, 1 sgs, 2 mg, 3 mgfw, 4 poly, 5 mgpoly.
 * Built per format: -DCRS and -DSCS.
 */
#include <ctype.h>
#include <stdlib.h>

#include "sparsebench/sparsebench.h"

int main(int argc, char** argv)
{
  if (argc < 6) {
    fprintf(stderr, "usage: %s <n | file.mtx> <itermax> <eps> <restart> <precond>\n", argv[0]);
    return 2;
  }
  Comm comm;
  Parameter param;
  commInit(&comm, argc, argv);
  initParameter(&param);
  param.itermax = atoi(argv[2]);
  param.eps     = atof(argv[3]);
  GMatrix m;
  if (isdigit((unsigned char)argv[1][0])) {
    param.nx = param.ny = param.nz = atoi(argv[1]);
    matrixGenerate(&m, &param, comm.rank, comm.size, false);
  } else {
    param.filename = argv[1];
    MMMatrix mm, local;
    memset(&mm, 0, sizeof mm), memset(&local, 0, sizeof local);
    MMMatrixRead(&mm, param.filename);
    commDistributeMatrix(&comm, &mm, &local);
    matrixConvertfromMM(&local, &m);
  }
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
  int k = solveGMRESPrecond(&comm, &param, &sm, atoi(argv[4]), atoi(argv[5]));
  printf("k %d\n", k);
  profilerPrint(&comm, k);
  profilerFinalize();
  commFinalize(&comm);
  return EXIT_SUCCESS;
}
