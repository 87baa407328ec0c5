/* sbh_main.c -- the benchmark driver: SparseBench's command line and output, HIP
 * hot path.  Built per format like the reference executable (sparseBench-<FMT>-HIP).
 * Follows src/main.c:83-230 call for call; differences:
 *   - every rank reads a .mtx itself (no MPI scatter), see commDistributeMatrix;
 *   - SCS gets -C <chunk height> and -s <sigma> (the reference has no flag, and no
 *     working SCS path);
 *   - -t spmv is the reference's own loop (allocate() + host loops + PROFILE(spMVM)); the allocation hook hands out
 *     HBM-resident, host-visible vectors, so the loop times the kernel (host/sbh_base.c);
 *   - .bmx files (-c <file.mtx> writes one, -m <file.bmx> loads one) go through plain
 *     POSIX I/O instead of MPI-IO (sbh_binfile.c); SB_BMX_FP64=1 keeps fp64 values;
 *   - the options are parsed and checked by sbh_parse_options (sbh_options.c), which needs no device: here is what it asks for.
 */
#define _GNU_SOURCE
#include <stdlib.h>

#include "sbhip.h"
#include "sparsebench/sparsebench.h"

int main(int argc, char** argv)
{
  Parameter param;
  Comm comm;
  commInit(&comm, argc, argv);
  initParameter(&param);
  sbh_options o;
  char msg[MAXLINE];
  int refused = sbh_parse_options(argc, argv, &param, &o, msg, sizeof msg);
  if (!refused && o.action == SBH_ACT_RUN) refused = sbh_check_ranks(&o, comm.size, msg, sizeof msg); /* (the launcher's ranks) */
  if (o.action == SBH_ACT_HELP) {
    if (commIsMaster(&comm)) printf("%s", sbh_help_text());
    commAbort(&comm, "");
  }
  if (o.action == SBH_ACT_CONVERT) {
    sbh_write_bin_matrix(&comm, o.convert); /* src/main.c:107-110 */
    commAbort(&comm, "Finish write matrix");
  }
  for (int i = o.optind; i < argc; i++) printf("Non-option argument %s\n", argv[i]);
  if (refused) {
    fputs(msg, o.toStdout ? stdout : stderr);
    return 1;
  }

  commPrintBanner(&comm);

  double ts;
  GMatrix m;
  double timeStart = getTimeStamp();
  sbh_init_matrix(&comm, &param, &m);
  commPartition(&comm, &m);
  Matrix sm;
  memset(&sm, 0, sizeof sm);
#ifdef SCS
  sm.C = o.scsC, sm.sigma = o.scsSigma;
#endif
  convertMatrix(&sm, &m);
  commBarrier();
  double timeStop = getTimeStamp();
  if (commIsMaster(&comm)) printf("Setup took %.2fs\n", timeStop - timeStart);

  size_t factorFlops[NUMREGIONS] = { 0 }, factorWords[NUMREGIONS] = { 0 };
  factorFlops[DDOT] = factorFlops[WAXPBY] = m.totalNr; /* src/main.c:181-190 */
  factorWords[DDOT] = factorWords[WAXPBY] = sizeof(CG_FLOAT) * (size_t)m.totalNr;
  factorFlops[SPMVM] = m.totalNnz;
  factorWords[SPMVM] = (sizeof(CG_FLOAT) + sizeof(CG_UINT)) * (size_t)m.totalNnz;
  profilerInit(factorFlops, factorWords);

  /* the add-on solvers: -t's type, the line that names it, and sbh_solve_precond's solver */
  static const struct {
    int type;
    const char* name;
    int solver;
  } addon[] = { { SBH_BENCH_GMRES, "GMRES", SBH_SOLVER_GMRES }, { SBH_BENCH_PCG, "PCG", SBH_SOLVER_PCG },
    { SBH_BENCH_BICGSTAB, "BiCGStab", SBH_SOLVER_BICGSTAB } };
  size_t a = 0;
  while (a < sizeof addon / sizeof *addon && addon[a].type != o.type) a++;
  int k = 0;
  if (o.type == SBH_BENCH_CG) {
    if (commIsMaster(&comm)) printf("Test type: CG\n");
    k = o.nrhs == 1 ? solveCG(&comm, &param, &sm) : solveCGBatch(&comm, &param, &sm, o.nrhs);
  } else if (a < sizeof addon / sizeof *addon) {
    if (commIsMaster(&comm)) printf("Test type: %s\n", addon[a].name);
    /* (every other preconditioner's line is the solve's own: it knows the colours, the levels, the interval) */
    const int jacobi = o.precond.kind == SBH_PRECOND_NONE || o.precond.kind == SBH_PRECOND_JACOBI;
    if (o.type == SBH_BENCH_PCG && jacobi && commIsMaster(&comm)) printf("Preconditioner: Jacobi (diagonal), nC = 0\n");
    k = sbh_solve_precond(&comm, &param, sm.dev, sm.nr, sm.rowNnz, SBH_FMT_ARGS(&sm), addon[a].solver, o.restart,
        o.precond.kind == SBH_PRECOND_NONE ? NULL : &o.precond);
  } else {
    if (commIsMaster(&comm)) printf("Test type: SPMVM\n");
    /* exactly the reference's loop (src/main.c:205-215): vectors from the allocation hook, filled by host loops, spMVM under
     * PROFILE.  allocate() hands out HBM-resident, host-visible memory (host/sbh_base.c), so the loop times the kernel. */
    CG_FLOAT* x = (CG_FLOAT*)allocate(ARRAY_ALIGNMENT, (size_t)m.nc * sizeof(CG_FLOAT));
    CG_FLOAT* y = (CG_FLOAT*)allocate(ARRAY_ALIGNMENT, (size_t)m.nr * sizeof(CG_FLOAT));
    for (CG_UINT i = 0; i < m.nc; i++) x[i] = (CG_FLOAT)1.0; /* (the reference leaves the halo tail uninitialised) */
    for (CG_UINT i = 0; i < m.nr; i++) y[i] = (CG_FLOAT)1.0;
    for (k = 1; k < param.itermax; k++) {
      PROFILE(SPMVM, spMVM(&sm, x, y));
    }
  }
  profilerPrint(&comm, k);
  profilerFinalize();
  commFinalize(&comm);
  return EXIT_SUCCESS;
}
