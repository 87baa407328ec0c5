/* dropin.c -- the link-time slot.  Compiled twice, -DCRS and -DSCS, into
 * libsparsebench_crs.so / libsparsebench_scs.so: each exports convertMatrix, spMVM and
 * solveCG for ITS Matrix typedef, exactly as the reference links one matrix-<FMT>.o
 * (reference Makefile:20,32-34; src/matrix.h:14-22,57; src/solver.h:11-13).
 */
#include <stdlib.h>

#include "sbhip.h"
#include "sparsebench/sparsebench.h"

int sbh_solve_cg_perm(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz,
    const CG_UINT* oldToNewPerm);

#if defined(CRS)

void convertMatrix(Matrix* m, GMatrix* im) { sbh_convert_crs(m, im); }

int solveCG(Comm* comm, Parameter* param, Matrix* m)
{
  return sbh_solve_cg_perm(comm, param, m->dev, m->nr, m->rowNnz, NULL);
}

#elif defined(SCS)

/* The reference's driver never sets C / sigma (src/main.c:173-174) and its
 * convertMatrix overwrites them (src/matrix-SCS.c:42-43).  Here: SPARSEBENCH_C /
 * SPARSEBENCH_SIGMA win if set; otherwise plausible caller values are honoured;
 * otherwise C = 64 (one wavefront per chunk), sigma = 1. */
static CG_UINT pick(const char* env, CG_UINT given, CG_UINT lo, CG_UINT hi, CG_UINT dflt)
{
  const char* v = getenv(env);
  if (v && atoi(v) > 0) return (CG_UINT)atoi(v);
  if (given >= lo && given <= hi) return given;
  return dflt;
}

void convertMatrix(Matrix* m, GMatrix* im)
{
  m->C     = pick("SPARSEBENCH_C", m->C, 1, 4096, 64);
  m->sigma = pick("SPARSEBENCH_SIGMA", m->sigma, 1, 1u << 24, 1);
  sbh_convert_scs(m, im);
}

int solveCG(Comm* comm, Parameter* param, Matrix* m)
{
  return sbh_solve_cg_perm(comm, param, m->dev, m->nr, m->rowNnz, m->oldToNewPerm);
}

#else
#error "compile with -DCRS or -DSCS"
#endif

/* nrhs CG solves on one pass over this build's Matrix per body (the _sp libraries: "batched CG: double precision only") */
int solveCGBatch(Comm* comm, Parameter* param, Matrix* m, int nrhs)
{
  return sbh_solve_cg_batch(comm, param, m->dev, m->nr, m->rowNnz, m->startRow, nrhs);
}

/* the add-on solvers on this build's Matrix, each preconditioner at its defaults (the _sp libraries: "<solver>: double precision
 * only"); spec NULL: the solver's own default */
static int solve(Comm* comm, Parameter* param, Matrix* m, int solver, int restart, const sbh_precond_spec* spec)
{
  return sbh_solve_precond(comm, param, m->dev, m->nr, m->rowNnz, SBH_FMT_ARGS(m), solver, restart, spec);
}
#define SPEC(kind, coarse) &(const sbh_precond_spec){ kind, 0, 0, coarse }
/* Jacobi-preconditioned CG; with multicolour symmetric Gauss-Seidel in the diagonal's place; with the multigrid V-cycle
 * around it on the generated grid's own hierarchy at auto depth (4.13); with full-weighting transfers between the levels (4.14) */
int solvePCG(Comm* comm, Parameter* param, Matrix* m) { return solve(comm, param, m, SBH_SOLVER_PCG, 0, NULL); }
int solvePCGSGS(Comm* comm, Parameter* param, Matrix* m) { return solve(comm, param, m, SBH_SOLVER_PCG, 0, SPEC(SBH_PRECOND_SGS, 0)); }
int solvePCGMG(Comm* comm, Parameter* param, Matrix* m) { return solve(comm, param, m, SBH_SOLVER_PCG, 0, SPEC(SBH_PRECOND_MG, 0)); }
int solvePCGMGFW(Comm* comm, Parameter* param, Matrix* m) { return solve(comm, param, m, SBH_SOLVER_PCG, 0, SPEC(SBH_PRECOND_MGFW, 0)); }
/* with the Chebyshev polynomial preconditioner (4.15); solvePCGMGFW with the polynomial as the smoother of every level (4.16); that on
 * Galerkin coarse operators formed on the device (4.17); that on the smoothed-aggregation hierarchy made from the matrix alone (4.19) */
int solvePCGPoly(Comm* comm, Parameter* param, Matrix* m) { return solve(comm, param, m, SBH_SOLVER_PCG, 0, SPEC(SBH_PRECOND_POLY, 0)); }
int solvePCGMGPoly(Comm* comm, Parameter* param, Matrix* m)
{
  return solve(comm, param, m, SBH_SOLVER_PCG, 0, SPEC(SBH_PRECOND_MGPOLY, SBH_COARSE_REGENERATED));
}
int solvePCGMGPolyGalerkin(Comm* comm, Parameter* param, Matrix* m)
{
  return solve(comm, param, m, SBH_SOLVER_PCG, 0, SPEC(SBH_PRECOND_MGPOLY, SBH_COARSE_GALERKIN));
}
int solvePCGMGPolySA(Comm* comm, Parameter* param, Matrix* m)
{
  return solve(comm, param, m, SBH_SOLVER_PCG, 0, SPEC(SBH_PRECOND_MGPOLY, SBH_COARSE_AGGREGATION));
}
/* Jacobi-preconditioned BiCGStab, or with one of PCG's preconditioners (4.18): 1 sgs, 2 mg, 3 mgfw, 4 poly, 5 mgpoly */
int solveBiCGStab(Comm* comm, Parameter* param, Matrix* m) { return solve(comm, param, m, SBH_SOLVER_BICGSTAB, 0, NULL); }
int solveBiCGStabPrecond(Comm* comm, Parameter* param, Matrix* m, int precond)
{
  return solve(comm, param, m, SBH_SOLVER_BICGSTAB, 0, SPEC(precond, 0));
}
/* restarted GMRES, or right-preconditioned by one of PCG's preconditioners (4.20): 0 jacobi, 1 sgs, 2 mg, 3 mgfw, 4 poly, 5 mgpoly */
int solveGMRES(Comm* comm, Parameter* param, Matrix* m, int restart) { return solve(comm, param, m, SBH_SOLVER_GMRES, restart, NULL); }
int solveGMRESPrecond(Comm* comm, Parameter* param, Matrix* m, int restart, int precond)
{
  return solve(comm, param, m, SBH_SOLVER_GMRES, restart, SPEC(precond, 0));
}
#undef SPEC

void sbh_print_banner(Comm* c, const char* fmt);
void commPrintBanner(Comm* c) { sbh_print_banner(c, FMT); } /* src/comm.c:185-250: names the build's format */

void spMVM(Matrix* m, const CG_FLOAT* restrict x, CG_FLOAT* restrict y)
{
  sbh_spmv(m->dev, m->nr, m->nc, x, y);
}

/* src/comm.h:55 (VERBOSE-build diagnostic): scalars of the converted matrix */
void commMatrixDump(Comm* c, Matrix* m)
{
  FILE* f = c->logFile ? c->logFile : stdout;
  fprintf(f, "Matrix (%s): rank %d, nr %u nc %u nnz %u totalNr %u totalNnz %u rows %u..%u\n", FMT, c->rank, m->nr,
      m->nc, m->nnz, m->totalNr, m->totalNnz, m->startRow, m->stopRow);
#if defined(SCS)
  fprintf(f, "C %u sigma %u nrPadded %u nChunks %u nElems %u\n", m->C, m->sigma, m->nrPadded, m->nChunks, m->nElems);
#endif
  fflush(f);
}
