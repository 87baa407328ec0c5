/* sbh_options.c -- the benchmark driver's command line (sbh_main.c), parsed and checked without a device: no Comm, no call
 * into the HIP layer, no exit, no output.  The driver prints what comes back; the tests call it as it stands.
 */
#define _GNU_SOURCE
#include <ctype.h>
#include <stdarg.h>
#include <stdlib.h>
#include <unistd.h>

#include "sparsebench/sparsebench.h"

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
    "  Several ranks: -t cg, -t spmv, and -t pcg with -p jacobi or -p poly [-d n]; every other preconditioner, -g, -a,\n"
    "             -t gmres and -t bicgstab run on one rank.\n"
    "  -r <int>   GMRES restart length. Default 30.\n"
    "  -n <int>   Number of right-hand sides for -t cg. Default 1.\n"
    "  -x <int>   Size in x for generated matrix, ignored if MM file is loaded. Default 100.\n"
    "  -y <int>   Size in y for generated matrix, ignored if MM file is loaded. Default 100.\n"
    "  -z <int>   Size in z for generated matrix, ignored if MM file is loaded. Default 100.\n"
    "  -i <int>   Number of solver iterations. Default 150.\n"
    "  -e <float>  Convergence criteria epsilon. Default 0.0.\n"
    "  -C <int>   Sell-C-sigma chunk height (SCS build). Default 64.\n"
    "  -s <int>   Sell-C-sigma sorting scope (SCS build). Default 1.\n";

const char* sbh_help_text(void) { return kHelp; }

/* -t's names; dp: the solver's name where the single-precision driver does not have it */
static const struct {
  const char* name;
  int type;
  const char* dp;
} kTypes[] = { { "cg", SBH_BENCH_CG, NULL }, { "spmv", SBH_BENCH_SPMV, NULL }, { "gmres", SBH_BENCH_GMRES, "GMRES" },
  { "pcg", SBH_BENCH_PCG, "PCG" }, { "bicgstab", SBH_BENCH_BICGSTAB, "BiCGStab" } };
/* -p's and -P's names, by SBH_PRECOND_* */
static const char* const kPrecond[] = { "jacobi", "sgs", "mg", "mgfw", "poly", "mgpoly" };
#if PRECISION == 1
static const int kSingle = 1;
#else
static const int kSingle = 0;
#endif

static int precond_kind(const char* name)
{
  for (int k = 0; k < (int)(sizeof kPrecond / sizeof *kPrecond); k++)
    if (strcmp(name, kPrecond[k]) == 0) return k;
  return SBH_PRECOND_NONE;
}

static int refuse(char* msg, size_t cap, const char* fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, cap, fmt, ap);
  va_end(ap);
  return 1;
}

int sbh_parse_options(int argc, char** argv, Parameter* param, sbh_options* o, char* msg, size_t cap)
{
  const sbh_options defaults = { SBH_BENCH_CG, 30, 1, 64, 1, 0, { SBH_PRECOND_NONE, 0, 0, SBH_COARSE_REGENERATED }, argc, SBH_ACT_RUN, NULL, 0 };
  *o = defaults;
  sbh_precond_spec* pc = &o->precond;
  int precond = SBH_PRECOND_NONE, bprecond = SBH_PRECOND_NONE; /* -p's and -P's */
  int galerkin = 0, aggregation = 0;                           /* -g, -a */
  int opt;
  if (cap) msg[0] = '\0';
  opterr = 0;
  optind = 0; /* (a fresh scan, whatever an earlier one left behind) */
  while ((opt = getopt(argc, argv, "hc:t:f:m:x:y:z:i:e:C:s:r:n:p:P:l:ad:g")) != -1) switch (opt) {
    case 'h': o->action = SBH_ACT_HELP; return 0;
    case 'c': /* src/main.c:107-110 */
      o->action  = SBH_ACT_CONVERT;
      o->convert = optarg;
      return 0;
    case 'f': readParameter(param, optarg); break;
    case 'm': param->filename = optarg; break;
    case 't': {
      size_t t = 0;
      while (t < sizeof kTypes / sizeof *kTypes && strcmp(optarg, kTypes[t].name) != 0) t++;
      if (t == sizeof kTypes / sizeof *kTypes) {
        o->toStdout = 1;
        return refuse(msg, cap, "Unknown solver type %s\n", optarg);
      }
      if (kSingle && kTypes[t].dp) return refuse(msg, cap, "%s: double precision only\n", kTypes[t].dp);
      o->type = kTypes[t].type;
      break;
    }
    case 'x': param->nx = atoi(optarg); break;
    case 'y': param->ny = atoi(optarg); break;
    case 'z': param->nz = atoi(optarg); break;
    case 'i': param->itermax = atoi(optarg); break;
    case 'e': param->eps = atof(optarg); break;
    case 'C': o->scsC = (unsigned)atoi(optarg); break;
    case 's': o->scsSigma = (unsigned)atoi(optarg); break;
    case 'r': o->restart = atoi(optarg); break;
    case 'n': o->nrhs = atoi(optarg); break;
    case 'p':
      if ((precond = precond_kind(optarg)) == SBH_PRECOND_NONE)
        return refuse(msg, cap, "Unknown preconditioner %s (-p <jacobi|sgs>)\n", optarg);
      break;
    case 'P': /* (jacobi with -t gmres only: refused below, where the type is known) */
      if ((bprecond = precond_kind(optarg)) == SBH_PRECOND_NONE)
        return refuse(msg, cap, "Unknown preconditioner %s (-P <sgs|mg|mgfw|poly|mgpoly>)\n", optarg);
      break;
    case 'l':
      pc->levels = atoi(optarg);
      if (pc->levels < 1)
        return refuse(msg, cap, "-l <int> (the levels of -p mg, -p mgfw or -p mgpoly) must be 1 or more, got %s\n", optarg);
      break;
    case 'g': galerkin = 1; break;
    case 'a': aggregation = 1; break;
    case 'd':
      pc->steps = atoi(optarg);
      if (pc->steps < 1 || pc->steps > 16)
        return refuse(msg, cap, "-d <int> (the steps of -p poly or -p mgpoly) must be 1 to 16, got %s\n", optarg);
      break;
    default:
      if (isprint(optopt)) return refuse(msg, cap, "Unknown option `-%c'.\n", optopt);
      return refuse(msg, cap, "Unknown option character `\\x%x'.\n", optopt);
    }
  o->optind = optind;
  const int type = o->type;
  if (o->nrhs != 1 && type != SBH_BENCH_CG) return refuse(msg, cap, "-n <int> (several right-hand sides) goes with -t cg only\n");
  if (precond != SBH_PRECOND_NONE && type != SBH_BENCH_PCG)
    return refuse(msg, cap, "-p <jacobi|sgs> (the preconditioner) goes with -t pcg only\n");
  if (bprecond == SBH_PRECOND_JACOBI && type != SBH_BENCH_GMRES) /* BiCGStab's diagonal is its default: -P names the plans there */
    return refuse(msg, cap, "Unknown preconditioner jacobi (-P <sgs|mg|mgfw|poly|mgpoly>)\n");
  if (bprecond != SBH_PRECOND_NONE && type != SBH_BENCH_BICGSTAB && type != SBH_BENCH_GMRES)
    return refuse(msg, cap, "-P <sgs|mg|mgfw|poly|mgpoly> (the preconditioner of BiCGStab) goes with -t bicgstab only, or as "
                            "-P <jacobi|sgs|mg|mgfw|poly|mgpoly> with -t gmres\n");
  o->byP   = bprecond != SBH_PRECOND_NONE; /* -l, -d, -g and the grid's refusals below take -P where they take -p */
  pc->kind = o->byP ? bprecond : precond;
  pc->coarse = aggregation ? SBH_COARSE_AGGREGATION : galerkin ? SBH_COARSE_GALERKIN : SBH_COARSE_REGENERATED;
  const int vcycle = pc->kind == SBH_PRECOND_MG || pc->kind == SBH_PRECOND_MGFW || pc->kind == SBH_PRECOND_MGPOLY;
  if (pc->levels != 0 && !vcycle) return refuse(msg, cap, "-l <int> (the levels) goes with -p mg only, or with -p mgfw or -p mgpoly\n");
  if (pc->steps != 0 && pc->kind != SBH_PRECOND_POLY && pc->kind != SBH_PRECOND_MGPOLY)
    return refuse(msg, cap, "-d <int> (the steps) goes with -p poly only, or with -p mgpoly\n");
  if (galerkin && pc->kind != SBH_PRECOND_MGPOLY) return refuse(msg, cap, "-g (Galerkin coarse operators) goes with -p mgpoly only\n");
  if (aggregation && pc->kind != SBH_PRECOND_MGPOLY)
    return refuse(msg, cap, "-a (smoothed-aggregation coarsening) goes with -p mgpoly only\n");
  if (aggregation && galerkin)
    return refuse(msg, cap, "-a (smoothed-aggregation coarsening) forms its own Galerkin products P^T A P on the device: it does not go with -g, "
                            "which is the trilinear hierarchy's\n");
  if (vcycle && !aggregation) { /* refused before the set-up: a file has no grid, a grid may not allow the levels */
    char why[256];
    if (!sbh_is_generated(param))
      return refuse(msg, cap, "-%c %s needs the grid: its hierarchy is the generated matrix's on coarser grids, not -m %s\n", o->byP ? 'P' : 'p',
          kPrecond[pc->kind], param->filename);
    if (!sbh_mg_levels(param->nx, param->ny, param->nz, pc->levels, why, sizeof why)) return refuse(msg, cap, "%s\n", why);
  }
  return 0;
}

/* what of the parsed options runs on `size` ranks: -t cg, -t spmv, and -t pcg with the Jacobi diagonal or -p poly
 * [-d n].  The sweeps, the V-cycles (with -g and -a), GMRES and BiCGStab are refused here with the messages of their solves */
int sbh_check_ranks(const sbh_options* o, int size, char* msg, size_t cap)
{
  if (cap) msg[0] = '\0';
  if (size < 2) return 0;
  if (o->type == SBH_BENCH_GMRES) return refuse(msg, cap, "GMRES: runs on one rank\n");
  if (o->type == SBH_BENCH_BICGSTAB) return refuse(msg, cap, "BiCGStab: runs on one rank\n");
  if (o->type != SBH_BENCH_PCG) return 0;
  switch (o->precond.kind) {
  case SBH_PRECOND_SGS: return refuse(msg, cap, "SGS: runs on one rank\n");
  case SBH_PRECOND_MG:
  case SBH_PRECOND_MGFW:
  case SBH_PRECOND_MGPOLY: return refuse(msg, cap, "MG: runs on one rank\n");
  default: return 0; /* the diagonal and the polynomial */
  }
}
