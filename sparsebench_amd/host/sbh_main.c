/* sbh_main.c -- the benchmark driver: SparseBench's command line and output, HIP
 * hot path.  Built per format like the reference executable (sparseBench-<FMT>-HIP).
 * Follows src/main.c:83-230 call for call; differences:
 *   - every rank reads a .mtx itself (no MPI scatter), see commDistributeMatrix;
 *   - SCS gets -C <chunk height> and -s <sigma> (the reference has no flag, and no
 *     working SCS path);
 *   - -t spmv is the reference's own loop (allocate() + host loops + PROFILE(spMVM)); the allocation hook hands out
 *     HBM-resident, host-visible vectors, so the loop times the kernel (host/sbh_base.c);
 *   - .bmx files (-c <file.mtx> writes one, -m <file.bmx> loads one) go through plain
 *     POSIX I/O instead of MPI-IO (sbh_binfile.c); SB_BMX_FP64=1 keeps fp64 values.
 */
#define _GNU_SOURCE
#include <ctype.h>
#include <stdlib.h>
#include <unistd.h>

#include "sbhip.h"
#include "sparsebench/sparsebench.h"

typedef enum { CG = 0, SPMV, GMRES, CHEBFD, PCG, BICGSTAB } bench_type;

static const char* kHelp =
    "Usage: sparseBench [options]\n\n"
    "Options:\n"
    "  -h         Show this help text\n"
    "  -f <parameter file>   Load options from a parameter file\n"
    "  -c <file name>   Convert MM matrix to binary matrix file (.bmx).\n"
    "  -m <matrix>   Load a matrix market (.mtx) or binary (.bmx) file\n"
    "  -t <bench type>   Benchmark type, can be cg, spmv, gmres, pcg (CG with the Jacobi preconditioner),\n"
    "                    or bicgstab (BiCGStab with the Jacobi preconditioner: non-symmetric matrices). Default cg.\n"
    "  -p <jacobi|sgs>   Preconditioner of -t pcg, sgs is multicolour symmetric Gauss-Seidel. Default jacobi.\n"
    "  -p mg      Multigrid V-cycle with the sgs smoother as the preconditioner of -t pcg (generated matrices).\n"
    "  -p mgfw    The same with full-weighting transfers: trilinear interpolation and its scaled transpose.\n"
    "  -l <int>   Levels of -p mg and -p mgfw. Default the deepest of up to 4 that the grid allows.\n"
    "  -p poly    Chebyshev polynomial in D^-1 A as the preconditioner of -t pcg: one SpMV per step behind the first.\n"
    "  -d <int>   Steps of -p poly, 1 to 16. Default 3.\n"
    "  -p mgpoly  The V-cycle of -p mgfw with that polynomial as the smoother of every level: no colouring.\n"
    "             Takes -l as -p mg does, and -d for the steps of each smoothing. Default 2.\n"
    "  -g         Galerkin coarse operators P^T A P, formed on the device, for -p mgpoly in the regenerated stencils' place.\n"
    "  -a         Smoothed-aggregation coarsening for -p mgpoly, made on the device from the matrix alone: any matrix (-m file,\n"
    "             -m irregular, generated). Forms its own Galerkin products (not with -g). Takes -l (default up to 4) and -d.\n"
    "  -P <sgs|mg|mgfw|poly|mgpoly>   One of those preconditioners for -t bicgstab in its diagonal's place, with -l, -d, -g, -a as for -p.\n"
    "             With -t gmres it is the right preconditioner of GMRES(m), and -P jacobi (the diagonal) is one more.\n"
    "  -r <int>   GMRES restart length. Default 30.\n"
    "  -n <int>   Number of right-hand sides for -t cg. Default 1.\n"
    "  -x <int>   Size in x for generated matrix, ignored if MM file is loaded. Default 100.\n"
    "  -y <int>   Size in y for generated matrix, ignored if MM file is loaded. Default 100.\n"
    "  -z <int>   Size in z for generated matrix, ignored if MM file is loaded. Default 100.\n"
    "  -i <int>   Number of solver iterations. Default 150.\n"
    "  -e <float>  Convergence criteria epsilon. Default 0.0.\n"
    "  -C <int>   Sell-C-sigma chunk height (SCS build). Default 64.\n"
    "  -s <int>   Sell-C-sigma sorting scope (SCS build). Default 1.\n";

/* the fmt, C, sigma arguments of the sbh_solve_* entries that rebuild the matrix on coarser grids, for this build's Matrix */
#ifdef SCS
#define SBH_FMT_ARGS(m) 1, (m)->C, (m)->sigma
#else
#define SBH_FMT_ARGS(m) 0, 0, 0
#endif

/* -p and -P number the preconditioners alike: optarg's number, -1 for a name that is none */
static int precond_number(void)
{
  if (strcmp(optarg, "jacobi") == 0) return 0;
  if (strcmp(optarg, "sgs") == 0) return 1;
  if (strcmp(optarg, "mg") == 0) return 2;
  if (strcmp(optarg, "mgfw") == 0) return 3;
  if (strcmp(optarg, "poly") == 0) return 4;
  if (strcmp(optarg, "mgpoly") == 0) return 5;
  return -1;
}

/* a solver the single-precision driver does not have: its message, exit status 1 */
static void dp_only(const char* msg)
{
#if PRECISION == 1
  fputs(msg, stderr);
  exit(1);
#else
  (void)msg;
#endif
}

int main(int argc, char** argv)
{
  Parameter param;
  Comm comm;
  commInit(&comm, argc, argv);
  initParameter(&param);
  int type = CG, opt;
  unsigned scsC = 64, scsSigma = 1;
  int restart = 30, nrhs = 1;
  int precond = -1; /* -p: 0 jacobi, 1 sgs, 2 mg, 3 mgfw, 4 poly, 5 mgpoly; -1 not given */
  int levels  = 0;  /* -l: levels of -p mg; 0 not given (the deepest of up to 4) */
  int steps   = 0;  /* -d: steps of -p poly or -p mgpoly; 0 not given (3, 2) */
  int galerkin = 0; /* -g: the coarse operators of -p mgpoly are P^T A P */
  int aggregation = 0; /* -a: the hierarchy of -p mgpoly is made from the matrix alone by smoothed aggregation */
  int bprecond = -1; /* -P: the plan preconditioner of -t bicgstab or -t gmres, numbered as -p (0 with -t gmres only); -1 not given */
  opterr = 0;
  while ((opt = getopt(argc, argv, "hc:t:f:m:x:y:z:i:e:C:s:r:n:p:P:l:ad:g")) != -1) switch (opt) {
    case 'h':
      if (commIsMaster(&comm)) printf("%s", kHelp);
      commAbort(&comm, "");
      break;
    case 'c':
      sbh_write_bin_matrix(&comm, optarg); /* src/main.c:107-110 */
      commAbort(&comm, "Finish write matrix");
      break;
    case 'f': readParameter(&param, optarg); break;
    case 'm': param.filename = optarg; break;
    case 't':
      if (strcmp(optarg, "cg") == 0) type = CG;
      else if (strcmp(optarg, "spmv") == 0) type = SPMV;
      else if (strcmp(optarg, "gmres") == 0) {
        dp_only("GMRES: double precision only\n");
        type = GMRES;
      } else if (strcmp(optarg, "pcg") == 0) {
        dp_only("PCG: double precision only\n");
        type = PCG;
      } else if (strcmp(optarg, "bicgstab") == 0) {
        dp_only("BiCGStab: double precision only\n");
        type = BICGSTAB;
      } else {
        printf("Unknown solver type %s\n", optarg);
        return 1;
      }
      break;
    case 'x': param.nx = atoi(optarg); break;
    case 'y': param.ny = atoi(optarg); break;
    case 'z': param.nz = atoi(optarg); break;
    case 'i': param.itermax = atoi(optarg); break;
    case 'e': param.eps = atof(optarg); break;
    case 'C': scsC = (unsigned)atoi(optarg); break;
    case 's': scsSigma = (unsigned)atoi(optarg); break;
    case 'r': restart = atoi(optarg); break;
    case 'n': nrhs = atoi(optarg); break;
    case 'p':
      if ((precond = precond_number()) < 0) {
        fprintf(stderr, "Unknown preconditioner %s (-p <jacobi|sgs>)\n", optarg);
        return 1;
      }
      break;
    case 'P': /* (jacobi with -t gmres only: refused below, where the type is known) */
      if ((bprecond = precond_number()) < 0) {
        fprintf(stderr, "Unknown preconditioner %s (-P <sgs|mg|mgfw|poly|mgpoly>)\n", optarg);
        return 1;
      }
      break;
    case 'l':
      levels = atoi(optarg);
      if (levels < 1) {
        fprintf(stderr, "-l <int> (the levels of -p mg, -p mgfw or -p mgpoly) must be 1 or more, got %s\n", optarg);
        return 1;
      }
      break;
    case 'g': galerkin = 1; break;
    case 'a': aggregation = 1; break;
    case 'd':
      steps = atoi(optarg);
      if (steps < 1 || steps > 16) {
        fprintf(stderr, "-d <int> (the steps of -p poly or -p mgpoly) must be 1 to 16, got %s\n", optarg);
        return 1;
      }
      break;
    default:
      if (isprint(optopt)) fprintf(stderr, "Unknown option `-%c'.\n", optopt);
      else fprintf(stderr, "Unknown option character `\\x%x'.\n", optopt);
      return 1;
    }
  for (int i = optind; i < argc; i++) printf("Non-option argument %s\n", argv[i]);
  if (nrhs != 1 && type != CG) {
    fprintf(stderr, "-n <int> (several right-hand sides) goes with -t cg only\n");
    return 1;
  }
  if (precond != -1 && type != PCG) {
    fprintf(stderr, "-p <jacobi|sgs> (the preconditioner) goes with -t pcg only\n");
    return 1;
  }
  if (bprecond == 0 && type != GMRES) { /* BiCGStab's diagonal is its default: -P names the plans there */
    fprintf(stderr, "Unknown preconditioner jacobi (-P <sgs|mg|mgfw|poly|mgpoly>)\n");
    return 1;
  }
  if (bprecond != -1 && type != BICGSTAB && type != GMRES) {
    fprintf(stderr, "-P <sgs|mg|mgfw|poly|mgpoly> (the preconditioner of BiCGStab) goes with -t bicgstab only, or as "
                    "-P <jacobi|sgs|mg|mgfw|poly|mgpoly> with -t gmres\n");
    return 1;
  }
  const int bicg = bprecond != -1; /* -l, -d, -g and the grid's refusals below take -P where they take -p */
  if (bicg) precond = bprecond;
  if (levels != 0 && precond != 2 && precond != 3 && precond != 5) {
    fprintf(stderr, "-l <int> (the levels) goes with -p mg only, or with -p mgfw or -p mgpoly\n");
    return 1;
  }
  if (steps != 0 && precond != 4 && precond != 5) {
    fprintf(stderr, "-d <int> (the steps) goes with -p poly only, or with -p mgpoly\n");
    return 1;
  }
  if (galerkin && precond != 5) {
    fprintf(stderr, "-g (Galerkin coarse operators) goes with -p mgpoly only\n");
    return 1;
  }
  if (aggregation && precond != 5) {
    fprintf(stderr, "-a (smoothed-aggregation coarsening) goes with -p mgpoly only\n");
    return 1;
  }
  if (aggregation && galerkin) {
    fprintf(stderr, "-a (smoothed-aggregation coarsening) forms its own Galerkin products P^T A P on the device: it does not go with -g, "
                    "which is the trilinear hierarchy's\n");
    return 1;
  }
  if ((precond == 2 || precond == 3 || precond == 5) && !aggregation) { /* refused before the set-up: a file has no grid, a grid may not allow the levels */
    char why[256];
    if (strcmp(param.filename, "generate") != 0 && strcmp(param.filename, "generate7P") != 0) {
      fprintf(stderr, "-%c %s needs the grid: its hierarchy is the generated matrix's on coarser grids, not -m %s\n", bicg ? 'P' : 'p',
          precond == 5 ? "mgpoly" : precond == 3 ? "mgfw" : "mg", param.filename);
      return 1;
    }
    if (!sbh_mg_levels(param.nx, param.ny, param.nz, levels, why, sizeof why)) {
      fprintf(stderr, "%s\n", why);
      return 1;
    }
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
  sm.C = scsC, sm.sigma = scsSigma;
#else
  (void)scsC, (void)scsSigma;
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

  int k = 0;
  if (type == CG) {
    if (commIsMaster(&comm)) printf("Test type: CG\n");
    k = nrhs == 1 ? solveCG(&comm, &param, &sm) : solveCGBatch(&comm, &param, &sm, nrhs);
  } else if (type == GMRES) {
    if (commIsMaster(&comm)) printf("Test type: GMRES\n");
    if (!bicg) k = solveGMRES(&comm, &param, &sm, restart);
    else if (levels == 0 && steps == 0 && !galerkin && !aggregation) k = solveGMRESPrecond(&comm, &param, &sm, restart, precond); /* (prints "Preconditioner: ..." itself) */
    else
      k = sbh_solve_gmres_precond(&comm, &param, sm.dev, sm.nr, sm.rowNnz, SBH_FMT_ARGS(&sm), restart, precond, levels, steps, aggregation ? 2 : galerkin);
  } else if (type == PCG) {
    if (commIsMaster(&comm)) printf("Test type: PCG\n");
    if (precond == 1) {
      k = solvePCGSGS(&comm, &param, &sm); /* (prints "Preconditioner: SGS ..., nC = <colours>" itself: it knows them) */
    } else if (precond == 2 && levels == 0) {
      k = solvePCGMG(&comm, &param, &sm); /* (prints "Preconditioner: MG ..., levels = L, nC = <colours>" itself) */
    } else if (precond == 2) {
      k = sbh_solve_pcg_mg(&comm, &param, sm.dev, sm.nr, sm.rowNnz, SBH_FMT_ARGS(&sm), levels);
    } else if (precond == 3 && levels == 0) {
      k = solvePCGMGFW(&comm, &param, &sm); /* (prints "Preconditioner: MG (V-cycle, full-weighting transfers, ..." itself) */
    } else if (precond == 3) {
      k = sbh_solve_pcg_mgfw(&comm, &param, sm.dev, sm.nr, sm.rowNnz, SBH_FMT_ARGS(&sm), levels);
    } else if (precond == 5 && aggregation && levels == 0 && steps == 0) {
      k = solvePCGMGPolySA(&comm, &param, &sm); /* (prints "Preconditioner: MG (V-cycle, ..., smoothed-aggregation coarsening), ..." itself) */
    } else if (precond == 5 && aggregation) {
      k = sbh_solve_pcg_mgpoly_sa(&comm, &param, sm.dev, sm.nr, sm.rowNnz, SBH_FMT_ARGS(&sm), levels, steps);
    } else if (precond == 5 && galerkin && levels == 0 && steps == 0) {
      k = solvePCGMGPolyGalerkin(&comm, &param, &sm); /* (prints "Preconditioner: MG (V-cycle, ..., Galerkin coarse operators), ..." itself) */
    } else if (precond == 5 && galerkin) {
      k = sbh_solve_pcg_mgpoly_galerkin(&comm, &param, sm.dev, sm.nr, sm.rowNnz, SBH_FMT_ARGS(&sm), levels, steps);
    } else if (precond == 5 && levels == 0 && steps == 0) {
      k = solvePCGMGPoly(&comm, &param, &sm); /* (prints "Preconditioner: MG (V-cycle, ..., Chebyshev polynomial smoother), ..." itself) */
    } else if (precond == 5) {
      k = sbh_solve_pcg_mgpoly(&comm, &param, sm.dev, sm.nr, sm.rowNnz, SBH_FMT_ARGS(&sm), levels, steps);
    } else if (precond == 4) { /* (prints "Preconditioner: Chebyshev polynomial, steps = ..., lambda in [...]" itself) */
      k = steps == 0 ? solvePCGPoly(&comm, &param, &sm) : sbh_solve_pcg_poly(&comm, &param, sm.dev, sm.nr, sm.rowNnz, steps);
    } else {
      if (commIsMaster(&comm)) printf("Preconditioner: Jacobi (diagonal), nC = 0\n");
      k = solvePCG(&comm, &param, &sm);
    }
  } else if (type == BICGSTAB) {
    if (commIsMaster(&comm)) printf("Test type: BiCGStab\n");
    if (!bicg) k = solveBiCGStab(&comm, &param, &sm);
    else if (levels == 0 && steps == 0 && !galerkin && !aggregation) k = solveBiCGStabPrecond(&comm, &param, &sm, precond); /* (prints "Preconditioner: ..." itself) */
    else
      k = sbh_solve_bicgstab_precond(&comm, &param, sm.dev, sm.nr, sm.rowNnz, SBH_FMT_ARGS(&sm), precond, levels, steps, aggregation ? 2 : galerkin);
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
