/* solver_driver.c -- a caller of one of the add-on solvers written ONLY against the reference-shaped API
 * (include/sparsebench/sparsebench.h): the set-up sequence of src/main.c:164-225 for a generated matrix or a Matrix Market
 * file, then the solver the build selects with exactly one of
 *   -DSOLVER_GMRES     solveGMRES     (the solver the reference's driver names and leaves empty)
 *   -DSOLVER_BATCH     solveCGBatch   (nrhs CG solves on one pass over the matrix per loop body)
 *   -DSOLVER_PCG       solvePCG       (CG with the Jacobi preconditioner)
 *   -DSOLVER_BICGSTAB  solveBiCGStab  (BiCGStab with the Jacobi preconditioner)
 *   -DSOLVER_PCG_SGS, _MG, _MGFW, _POLY, _MGPOLY, _MGPOLY_GALERKIN, _MGPOLY_SA
 *                      solvePCGSGS, solvePCGMG, solvePCGMGFW, solvePCGPoly, solvePCGMGPoly, solvePCGMGPolyGalerkin, solvePCGMGPolySA
 *                      (CG with that preconditioner at its defaults)
 * Usage: solver_driver <n | file.mtx> <itermax> <eps> [<restart> | <nrhs>]: a first argument that starts with a digit generates
 * the n^3 grid, any other is read as a Matrix Market file; the fourth argument goes with GMRES (restart) and the batch (nrhs).
 * Built twice per solver: -DCRS and -DSCS.
 */
#include <ctype.h>
#include <stdlib.h>

#include "sparsebench/sparsebench.h"

#if defined(SOLVER_GMRES)
#define USAGE "<file.mtx> <itermax> <eps> <restart>"
#define EXTRA 1
#define SOLVE(comm, param, sm, extra) solveGMRES(comm, param, sm, extra)
#elif defined(SOLVER_BATCH)
#define USAGE "<n> <itermax> <eps> <nrhs>"
#define EXTRA 1
#define SOLVE(comm, param, sm, extra) solveCGBatch(comm, param, sm, extra)
#elif defined(SOLVER_PCG)
#define USAGE "<n | file.mtx> <itermax> <eps>"
#define EXTRA 0
#define SOLVE(comm, param, sm, extra) solvePCG(comm, param, sm)
#elif defined(SOLVER_BICGSTAB)
#define USAGE "<n | file.mtx> <itermax> <eps>"
#define EXTRA 0
#define SOLVE(comm, param, sm, extra) solveBiCGStab(comm, param, sm)
#else
#if defined(SOLVER_PCG_SGS)
#define PCG_ENTRY solvePCGSGS
#elif defined(SOLVER_PCG_MG)
#define PCG_ENTRY solvePCGMG
#elif defined(SOLVER_PCG_MGFW)
#define PCG_ENTRY solvePCGMGFW
#elif defined(SOLVER_PCG_POLY)
#define PCG_ENTRY solvePCGPoly
#elif defined(SOLVER_PCG_MGPOLY)
#define PCG_ENTRY solvePCGMGPoly
#elif defined(SOLVER_PCG_MGPOLY_GALERKIN)
#define PCG_ENTRY solvePCGMGPolyGalerkin
#elif defined(SOLVER_PCG_MGPOLY_SA)
#define PCG_ENTRY solvePCGMGPolySA
#else
#error "define one of SOLVER_GMRES, SOLVER_BATCH, SOLVER_PCG, SOLVER_BICGSTAB, SOLVER_PCG_<preconditioner>"
#endif
#define USAGE "<n | file.mtx> <itermax> <eps>"
#define EXTRA 0
#define SOLVE(comm, param, sm, extra) PCG_ENTRY(comm, param, sm)
#endif

int main(int argc, char** argv)
{
  if (argc < 4 + EXTRA) {
    fprintf(stderr, "usage: %s " USAGE "\n", argv[0]);
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
  int k = SOLVE(&comm, &param, &sm, atoi(argv[4]));
  printf("k %d\n", k);
  profilerPrint(&comm, k);
  profilerFinalize();
  commFinalize(&comm);
  return EXIT_SUCCESS;
}
