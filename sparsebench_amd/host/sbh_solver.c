/* sbh_solver.c -- the C side of the solver API: solveCG, spMVM, waxpby, ddot with the
 * reference's signatures (src/solver.h:11-25), each a thin call into the HIP layer.
 * Also the profiler table (src/profiler.c) because solveCG feeds it.
 *
 * Pointer convention: hot-path vectors live in HBM (sb_malloc).  A host pointer is
 * accepted everywhere the reference's own driver passes one (src/main.c:205-215
 * allocates x, y with sbh_alloc_host()): it is staged through HBM -- still computed on the
 * GPU, just slower.  Nothing here computes on the CPU.
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdlib.h>

#include "sbhip.h"
#include "sparsebench/sparsebench.h"

void sbh_comm_attach_halo(Comm* c, CG_UINT nr, const CG_UINT* oldToNewPerm);

double _t[NUMREGIONS];

void sbh_profile_sync(void)
{
  if (sb_is_initialized()) sb_sync();
}

/* PROFILE's device-timed regions (include/sparsebench/sparsebench.h); no-ops until a device is up */
void sbh_region_begin(int tag)
{
  if (sb_is_initialized()) sb_region_begin(tag);
}
void sbh_region_end(int tag)
{
  if (sb_is_initialized()) sb_region_end(tag);
}

/* ---- staging helpers --------------------------------------------------------------- */
typedef struct {
  const void* host;
  CG_FLOAT* dev;
  int staged;
} staged_vec;

static staged_vec stage_in(const CG_FLOAT* p, size_t n, int copy)
{
  staged_vec s = { p, (CG_FLOAT*)p, 0 };
  if (n == 0 || sb_is_device_ptr(p)) return s;
  s.dev    = (CG_FLOAT*)sb_malloc(n * sizeof(CG_FLOAT));
  s.staged = 1;
  if (copy) sb_h2d(s.dev, p, n * sizeof(CG_FLOAT));
  return s;
}

static void stage_out(staged_vec* s, CG_FLOAT* host, size_t n)
{
  if (!s->staged) return;
  if (host) sb_d2h(host, s->dev, n * sizeof(CG_FLOAT));
  sb_free(s->dev);
}

/* ---- kernels with the reference's names ---------------------------------------------- */
void waxpby(const CG_UINT n, const CG_FLOAT alpha, const CG_FLOAT* restrict x, const CG_FLOAT beta,
    const CG_FLOAT* restrict y, CG_FLOAT* w)
{
  staged_vec sx = stage_in(x, n, 1);
  staged_vec sy = (y == x) ? sx : stage_in(y, n, 1);
  staged_vec sw = (w == x) ? sx : (w == y) ? sy : stage_in(w, n, 0);
  SBH_FP(sb_waxpby)(n, alpha, sx.dev, beta, sy.dev, sw.dev);
  if (sw.staged) sb_d2h(w, sw.dev, (size_t)n * sizeof(CG_FLOAT));
  if (sw.staged && w != x && w != y) sb_free(sw.dev);
  if (sy.staged && y != x) sb_free(sy.dev);
  if (sx.staged) sb_free(sx.dev);
}

void ddot(const CG_UINT n, const CG_FLOAT* restrict x, const CG_FLOAT* restrict y,
    CG_FLOAT* restrict result)
{
  staged_vec sx = stage_in(x, n, 1);
  staged_vec sy = (y == x) ? sx : stage_in(y, n, 1);
  *result       = SBH_FP(sb_ddot)(n, sx.dev, sy.dev); /* process default dot order; includes the SUM all-reduce (src/solver.c:60) */
  if (sy.staged && y != x) sb_free(sy.dev);
  if (sx.staged) sb_free(sx.dev);
}

void sbh_spmv(void* dev_matrix, CG_UINT nr, CG_UINT nc, const CG_FLOAT* x, CG_FLOAT* y)
{
  staged_vec sx = stage_in(x, nc, 1);
  staged_vec sy = stage_in(y, nr, 0);
  SBH_FP(sb_spmv)((const sb_matrix*)dev_matrix, sx.dev, sy.dev);
  stage_out(&sy, y, nr);
  stage_out(&sx, NULL, nc);
}

/* ---- what the solvers below share around their sb_*_solve -------------------------------- */
/* All but solveCG exist in the double-precision libraries only: the single-precision build refuses at the call. */
static void dp_only(const char* msg)
{
#if PRECISION == 1
  fputs(msg, stderr);
  exit(EXIT_FAILURE);
#else
  (void)msg;
#endif
}

/* initVectors, src/CGSolver.c:25-36, into fresh host arrays: *b has room for ncols right-hand sides of nr rows (the first one
 * is filled), *xexact is NULL for a matrix that was read from a file */
static void init_vectors_dp(const Parameter* param, CG_UINT nr, const CG_UINT* rowNnz, int ncols, double** b, double** xexact)
{
  const int generated = sbh_is_generated(param);
  *b                  = (double*)sbh_alloc_host(ARRAY_ALIGNMENT, ((size_t)nr * ncols + 1) * sizeof(double));
  *xexact             = generated ? (double*)sbh_alloc_host(ARRAY_ALIGNMENT, ((size_t)nr + 1) * sizeof(double)) : NULL;
  for (CG_UINT i = 0; i < nr; i++) {
    if (generated) {
      (*b)[i]      = 27.0 - ((double)((int)rowNnz[i] - 1));
      (*xexact)[i] = 1.0;
    } else {
      (*b)[i] = 1.0;
    }
  }
}

static int print_freq(int itermax) /* src/CGSolver.c:85-91 */
{
  const int f = itermax / 10;
  return f > 50 ? 50 : f < 1 ? 1 : f;
}

/* The lines solveCG prints while iterating (src/CGSolver.c:100,:116-118) for a solve that left its loop at k, from a recorded
 * history v of n entries.  rr != 0: v holds r.r, iteration j shows the residual it starts from, sqrt(v[j - 1]).  rr == 0: v
 * holds GMRES's residual estimates, iteration j shows the one after its step, v[j]. */
static void print_history(Comm* comm, const char* prefix, int k, int itermax, const double* v, int n, int rr)
{
  if (!commIsMaster(comm)) return;
  const int printFreq = print_freq(itermax);
  printf("%sInitial Residual = %E\n", prefix, n > 0 ? (rr ? sqrt(v[0]) : v[0]) : 0.0);
  for (int j = 1; j < k; j++)
    if (j % printFreq == 0 || j + 1 == itermax) {
      const int idx = rr ? j - 1 : j;
      if (idx < n) printf("%sIteration = %d Residual = %E\n", prefix, j, rr ? sqrt(v[idx]) : v[idx]);
    }
}

/* solveCG's closing line and solverCheckResidual's (:40-60); the loop's kernels overlap regions, so the profiler table's SpMV
 * row carries the loop */
static void print_tail(Comm* comm, int k, double loop_ms, int have_exact, double diff)
{
  if (commIsMaster(comm)) {
    printf("Solution performed %d iterations and took %.2fs\n", k, 1e-3 * loop_ms);
    if (have_exact) printf("Difference between computed and exact  = %f\n", diff);
  }
  _t[SPMVM] += 1e-3 * loop_ms;
}

/* ---- solveCG --------------------------------------------------------------------------- */
/* src/CGSolver.c:62-141.  The whole loop runs in the HIP layer without host round
 * trips; the lines the reference prints while iterating are printed afterwards from
 * the recorded history (same text, same order). */
static int sbh_solve(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz,
    const CG_UINT* oldToNewPerm)
{
  const int itermax    = param->itermax;
  const int generated  = sbh_is_generated(param);
  CG_FLOAT* b          = (CG_FLOAT*)sbh_alloc_host(ARRAY_ALIGNMENT, ((size_t)nr + 1) * sizeof(CG_FLOAT));
  CG_FLOAT* xexact     = generated ? (CG_FLOAT*)sbh_alloc_host(ARRAY_ALIGNMENT, ((size_t)nr + 1) * sizeof(CG_FLOAT)) : NULL;
  /* initVectors, src/CGSolver.c:25-36 */
  for (CG_UINT i = 0; i < nr; i++) {
    if (generated) {
      b[i]      = 27.0 - ((CG_FLOAT)((int)rowNnz[i] - 1));
      xexact[i] = 1.0;
    } else {
      b[i] = 1.0;
    }
  }
  sbh_comm_attach_halo(comm, nr, oldToNewPerm);
  /* the dot order is the process default (SB_DOT_ORDER / sb_set_dot_order): seq runs the reference's op list with its
   * sequential ddot, and the history -- the lines printed below -- is then the reference's bit for bit */
  sb_cg* cg = SBH_FP(sb_cg_create)((const sb_matrix*)dev_matrix, (sb_halo*)comm->dev, b, xexact);
  const char* fused = getenv("SB_FUSED");
  const char* graph = getenv("SB_GRAPH");
  if (fused) sb_cg_set_fused(cg, atoi(fused));
  if (graph) sb_cg_set_graph(cg, atoi(graph));

  const int k = sb_cg_solve(cg, itermax, param->eps);

  const int cap = itermax + 2;
  double* rr    = (double*)malloc((size_t)cap * sizeof(double));
  double* pAp   = (double*)malloc((size_t)cap * sizeof(double));
  int nPAp      = 0;
  const int nRr = sb_cg_history(cg, rr, cap, pAp, cap, &nPAp);
  const int printFreq = print_freq(itermax);
  if (commIsMaster(comm)) {
    /* normr is a CG_FLOAT: sqrt in double, stored to CG_FLOAT (src/CGSolver.c:100,116) */
    printf("Initial Residual = %E\n", nRr > 0 ? (CG_FLOAT)sqrt(rr[0]) : 0.0);
    /* iteration j's residual is sqrt of the r.r entering it: rr[0] for j = 1, rr[j-1] after */
    for (int j = 1; j < k; j++)
      if (j % printFreq == 0 || j + 1 == itermax) {
        const int idx = j == 1 ? 0 : j - 1;
        if (idx < nRr) printf("Iteration = %d Residual = %E\n", j, (CG_FLOAT)sqrt(rr[idx]));
      }
    printf("Solution performed %d iterations and took %.2fs\n", k, 1e-3 * sb_cg_loop_ms(cg));
  }
  /* solverCheckResidual, :40-60 */
  if (xexact) {
    const double diff = sb_cg_check_residual(cg);
    if (commIsMaster(comm)) printf("Difference between computed and exact  = %f\n", diff);
  }
  double ms[4];
  sb_cg_region_ms(cg, ms);
  double sum = ms[0] + ms[1] + ms[2] + ms[3];
  if (sum > 0.0) {
    _t[WAXPBY] += 1e-3 * ms[0], _t[SPMVM] += 1e-3 * ms[1], _t[DDOT] += 1e-3 * ms[2], _t[COMM] += 1e-3 * ms[3];
  } else {
    /* fused run: regions overlap inside kernels; attribute the loop to the SpMV row so
     * the table still adds up (run with SB_FUSED=0 or SB_DOT_ORDER=seq for the per-region split) */
    _t[SPMVM] += 1e-3 * sb_cg_loop_ms(cg);
  }
  sb_cg_free(cg);
  free(rr), free(pAp), free(b), free(xexact);
  return k;
}

int sbh_solve_cg(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz)
{
  return sbh_solve(comm, param, dev_matrix, nr, rowNnz, NULL);
}

int sbh_solve_cg_perm(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz,
    const CG_UINT* oldToNewPerm)
{
  return sbh_solve(comm, param, dev_matrix, nr, rowNnz, oldToNewPerm);
}

/* ---- solveGMRES -------------------------------------------------------------------------- */
/* The solver src/main.c:31,217-222 names and leaves empty.  The loop runs in the HIP layer (sb_gmres_*); the lines solveCG
 * prints while iterating are printed afterwards from the recorded history: iteration j shows the residual estimate after
 * the step taken at counter j. */
/* solves with the handle, prints, releases it and the vectors */
static int run_gmres(Comm* comm, Parameter* param, sb_gmres* s, double* b, double* xexact)
{
  const int itermax = param->itermax, cap = itermax + 2;
  const char* fused = getenv("SB_FUSED");
  if (fused) sb_gmres_set_fused(s, atoi(fused));
  const int k    = sb_gmres_solve(s, itermax, param->eps);
  double* res    = (double*)malloc((size_t)cap * sizeof(double));
  double* rr     = (double*)malloc((size_t)cap * sizeof(double));
  int nRr        = 0;
  const int nRes = sb_gmres_history(s, res, cap, rr, cap, &nRr);
  print_history(comm, "", k, itermax, res, nRes, 0);
  print_tail(comm, k, sb_gmres_loop_ms(s), xexact != NULL, sb_gmres_check_residual(s));
  sb_gmres_free(s);
  free(res), free(rr), free(b), free(xexact);
  return k;
}

/* ---- solveCGBatch ------------------------------------------------------------------------ */
/* nrhs independent CG solves whose loop bodies share one stream of the matrix (sb_cgb_*).  Column 0 is solveCG's
 * system; column c >= 1 has b_c[i] = b_0[i] + c * ((g(i) mod 5) - 2), g = startRow + i (small integers: exact).  The lines
 * solveCG prints come per column, prefixed "RHS c: ", from the recorded histories. */
int sbh_solve_cg_batch(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, CG_UINT startRow, int nrhs)
{
  dp_only("batched CG: double precision only\n");
  const int itermax = param->itermax, cap = itermax + 2;
  const int nv      = nrhs > 0 ? nrhs : 1; /* (a width the layer does not have is refused by sb_cgb_create, with its message) */
  double *B, *xexact;
  init_vectors_dp(param, nr, rowNnz, nv, &B, &xexact);
  for (int c = 1; c < nv; c++)
    for (CG_UINT i = 0; i < nr; i++) B[(size_t)c * nr + i] = B[i] + (double)c * (double)((int)(((size_t)startRow + i) % 5) - 2);
  sb_cgb* s   = sb_cgb_create((const sb_matrix*)dev_matrix, NULL, nrhs, B, xexact);
  const int k = sb_cgb_solve(s, itermax, param->eps);
  double* rr  = (double*)malloc((size_t)cap * sizeof(double));
  double* pAp = (double*)malloc((size_t)cap * sizeof(double));
  if (commIsMaster(comm)) {
    for (int c = 0; c < nv; c++) {
      char prefix[32];
      snprintf(prefix, sizeof prefix, "RHS %d: ", c);
      int nPAp      = 0;
      const int nRr = sb_cgb_history(s, c, rr, cap, pAp, cap, &nPAp);
      const int kc  = sb_cgb_iterations(s, c);
      print_history(comm, prefix, kc, itermax, rr, nRr, 1);
      printf("RHS %d: Solution performed %d iterations\n", c, kc);
    }
  }
  /* (the difference is for column 0, the one that has an exact solution) */
  print_tail(comm, k, sb_cgb_loop_ms(s), xexact != NULL, sb_cgb_check_residual(s, 0));
  sb_cgb_free(s);
  free(rr), free(pAp), free(B), free(xexact);
  return k;
}

/* ---- solvePCG and its preconditioners -------------------------------------------------------- */
/* solveCG with a preconditioner (sb_pcg_*): solves with the handle, prints solveCG's lines afterwards from the
 * recorded r.r history, indexed as solveCG's own, releases the handle and the vectors */
static int run_pcg(Comm* comm, Parameter* param, sb_pcg* s, double* b, double* xexact)
{
  const int itermax = param->itermax, cap = itermax + 2;
  const int k   = sb_pcg_solve(s, itermax, param->eps);
  double* rr    = (double*)malloc((size_t)cap * sizeof(double));
  double* rz    = (double*)malloc((size_t)cap * sizeof(double));
  double* pAp   = (double*)malloc((size_t)cap * sizeof(double));
  int nPAp      = 0;
  const int nRr = sb_pcg_history(s, rr, cap, rz, cap, pAp, cap, &nPAp);
  print_history(comm, "", k, itermax, rr, nRr, 1);
  print_tail(comm, k, sb_pcg_loop_ms(s), xexact != NULL, sb_pcg_check_residual(s));
  sb_pcg_free(s);
  free(rr), free(rz), free(pAp), free(b), free(xexact);
  return k;
}
/* the coarse levels of a V-cycle handle and the arrays they were built through: released after the handle (all NULL for the
 * one-level preconditioners) */
typedef struct {
  void* hierarchy;
  int fmt, L;
  const void** mats;
  const CG_UINT** maps;
  const uint64_t** gptr;
  const CG_UINT** gcol;
  const double** gval;
  double* gms;
} pcg_levels;
/* room for a hierarchy of up to maxL levels, ms_per_level stage times each; L is set once it is built */
static void pcg_levels_alloc(pcg_levels* H, int fmt, int maxL, int ms_per_level)
{
  memset(H, 0, sizeof *H);
  H->fmt  = fmt;
  H->mats = (const void**)calloc((size_t)maxL, sizeof *H->mats);
  H->maps = (const CG_UINT**)calloc((size_t)maxL, sizeof *H->maps);
  H->gptr = (const uint64_t**)calloc((size_t)maxL, sizeof *H->gptr);
  H->gcol = (const CG_UINT**)calloc((size_t)maxL, sizeof *H->gcol);
  H->gval = (const double**)calloc((size_t)maxL, sizeof *H->gval);
  H->gms  = (double*)calloc((size_t)ms_per_level * (size_t)maxL, sizeof *H->gms);
}
static void pcg_levels_free(pcg_levels* H)
{
  if (H->hierarchy) sbh_mg_hierarchy_free(H->hierarchy, H->fmt, H->L);
  free(H->mats), free(H->maps), free(H->gptr), free(H->gcol), free(H->gval), free(H->gms);
  memset(H, 0, sizeof *H);
}

static void mg_refuse(const char* msg)
{
  fprintf(stderr, "%s\n", msg);
  exit(EXIT_FAILURE);
}
/* the Chebyshev-smoothed V-cycle over the L levels of H with the prolongations ptr, col, val and the restriction's scale omega
 * between every two levels; steps per smoothing, 0: the default 2 (ratio 4) */
static sb_pcg* create_mg_poly(const sb_matrix* m, const double* b, const double* xexact, const pcg_levels* H, const uint64_t* const* ptr,
    const CG_UINT* const* col, const double* const* val, double omega, int steps)
{
  double* om = (double*)calloc((size_t)H->L, sizeof *om);
  for (int l = 0; l + 1 < H->L; l++) om[l] = omega;
  sb_pcg* s = sb_pcg_create_mg_poly(m, NULL, b, xexact, H->L - 1, (const sb_matrix* const*)H->mats, ptr, (const uint32_t* const*)col, val, om,
      steps ? steps : 2, 0, 0.0, 0.0);
  free(om);
  return s;
}

/* The V-cycle handles on the generated grid's own hierarchy (sbh_mg.c), with their "Preconditioner: ..." line.
 * spec->levels: L, or 0 for the deepest of up to 4 the grid allows.  mg: injection.  mgfw: the trilinear prolongations and omega =
 * 0.5 in the injection maps' place.  mgpoly: those prolongations with omega = 0.25 and the Chebyshev polynomial as the
 * smoother, or (SBH_COARSE_GALERKIN) the same on Galerkin coarse operators formed on the device, omega = 1.0
 *  */
static sb_pcg* build_pcg_mg(Comm* comm, Parameter* param, void* dev_matrix, const double* b, const double* xexact, int fmt, CG_UINT C,
    CG_UINT sigma, const sbh_precond_spec* spec, pcg_levels* H)
{
  if (!sbh_is_generated(param))
    mg_refuse("MG: needs the grid: the hierarchy is the generator's on coarser grids, and the matrix was read from a file "
              "(sb_pcg_create_mg takes a caller's own hierarchy)");
  if (comm->size > 1) mg_refuse("MG: runs on one rank");
  char why[256];
  const int L = sbh_mg_levels(param->nx, param->ny, param->nz, spec->levels, why, sizeof why);
  if (!L) mg_refuse(why);
  const sb_matrix* m = (const sb_matrix*)dev_matrix;
  const int poly     = spec->kind == SBH_PRECOND_MGPOLY;
  const int galerkin = poly && spec->coarse == SBH_COARSE_GALERKIN;
  pcg_levels_alloc(H, fmt, L, 2);
  H->hierarchy = galerkin ? sbh_mg_hierarchy_build_galerkin(param, dev_matrix, fmt, C, sigma, L, H->mats, H->gptr, H->gcol, H->gval, H->gms)
                          : sbh_mg_hierarchy_build(param, fmt, C, sigma, L, H->mats, H->maps);
  H->L = L;
  sb_pcg* s;
  if (galerkin) {
    s = create_mg_poly(m, b, xexact, H, H->gptr, H->gcol, H->gval, 1.0, spec->steps);
  } else if (spec->kind != SBH_PRECOND_MG) {
    uint64_t** ptr  = (uint64_t**)calloc((size_t)L, sizeof *ptr);
    CG_UINT** col   = (CG_UINT**)calloc((size_t)L, sizeof *col);
    double** val    = (double**)calloc((size_t)L, sizeof *val);
    double* omega   = (double*)calloc((size_t)L, sizeof *omega);
    int nx = param->nx, ny = param->ny, nz = param->nz;
    for (int l = 0; l + 1 < L; l++, nx /= 2, ny /= 2, nz /= 2) {
      const size_t n = (size_t)nx * ny * nz;
      ptr[l] = (uint64_t*)malloc((n + 1) * sizeof(uint64_t)), col[l] = (CG_UINT*)malloc(8 * n * sizeof(CG_UINT));
      val[l] = (double*)malloc(8 * n * sizeof(double)), omega[l] = 0.5;
      sbh_mg_trilinear(nx, ny, nz, ptr[l], col[l], val[l]);
    }
    if (poly)
      s = create_mg_poly(m, b, xexact, H, (const uint64_t* const*)ptr, (const CG_UINT* const*)col, (const double* const*)val, 0.25, spec->steps);
    else
      s = sb_pcg_create_mg_p(m, NULL, b, xexact, L - 1, (const sb_matrix* const*)H->mats, (const uint64_t* const*)ptr,
          (const uint32_t* const*)col, (const double* const*)val, omega);
    for (int l = 0; l + 1 < L; l++) free(ptr[l]), free(col[l]), free(val[l]);
    free(ptr), free(col), free(val), free(omega);
  } else {
    s = sb_pcg_create_mg(m, NULL, b, xexact, L - 1, (const sb_matrix* const*)H->mats, H->maps);
  }
  if (poly && commIsMaster(comm)) {
    double iv[2];
    sb_pcg_mg_poly_interval(s, 0, iv);
    printf("Preconditioner: MG (V-cycle, full-weighting transfers, Chebyshev polynomial smoother%s), levels = %d, steps = %d, "
           "lambda in [%.6g, %.6g]\n", galerkin ? ", Galerkin coarse operators" : "", sb_pcg_levels(s), sb_pcg_poly_steps(s), iv[0], iv[1]);
    if (galerkin) {
      printf("Galerkin products P^T A P on the device, ms (A P + P^T (A P)):");
      for (int l = 1; l < L; l++) printf(" level %d: %.3f + %.3f%s", l, H->gms[2 * (l - 1)], H->gms[2 * (l - 1) + 1], l + 1 < L ? "," : "");
      printf("\n");
    }
  } else if (commIsMaster(comm))
    printf("Preconditioner: MG (V-cycle, %smulticolour SGS smoother), levels = %d, nC = %d\n",
        spec->kind == SBH_PRECOND_MGFW ? "full-weighting transfers, " : "", sb_pcg_levels(s), sb_pcg_colours(s));
  return s;
}

/* The Chebyshev-smoothed V-cycle on the smoothed-aggregation hierarchy made from the matrix alone: any square
 * matrix, theta = 0, omega_s = 4/3, omega = 1.0; spec->levels 0: up to SBH_MG_SA_DEPTH */
static sb_pcg* build_pcg_sa(Comm* comm, void* dev_matrix, CG_UINT nr, const double* b, const double* xexact, int fmt, CG_UINT C,
    CG_UINT sigma, const sbh_precond_spec* spec, pcg_levels* H)
{
  if (comm->size > 1) mg_refuse("MG: runs on one rank");
  const int maxL  = spec->levels ? spec->levels : SBH_MG_SA_DEPTH;
  CG_UINT* rows   = (CG_UINT*)calloc((size_t)maxL, sizeof *rows);
  CG_UINT* rounds = (CG_UINT*)calloc((size_t)maxL, sizeof *rounds);
  int L           = 1;
  pcg_levels_alloc(H, fmt, maxL, 3);
  H->hierarchy = sbh_mg_hierarchy_build_sa(dev_matrix, nr, fmt, C, sigma, maxL, 0.0, 4.0 / 3.0, &L, H->mats, H->gptr, H->gcol, H->gval, rows,
      rounds, H->gms);
  H->L      = L;
  sb_pcg* s = create_mg_poly((const sb_matrix*)dev_matrix, b, xexact, H, H->gptr, H->gcol, H->gval, 1.0, spec->steps);
  if (commIsMaster(comm)) {
    double iv[2];
    sb_pcg_mg_poly_interval(s, 0, iv);
    printf("Preconditioner: MG (V-cycle, full-weighting transfers, Chebyshev polynomial smoother, smoothed-aggregation coarsening), "
           "levels = %d, steps = %d, lambda in [%.6g, %.6g]\n", sb_pcg_levels(s), sb_pcg_poly_steps(s), iv[0], iv[1]);
    printf("Aggregation on the device, rows:");
    for (int l = 0; l < L; l++) printf(" %u", rows[l]);
    printf("; rounds:");
    for (int l = 0; l + 1 < L; l++) printf(" %u", rounds[l]);
    printf("\n");
    printf("Aggregation set-up on the device, ms (aggregates + A T and smoothing + P^T A P):");
    for (int l = 0; l + 1 < L; l++)
      printf(" level %d: %.3f + %.3f + %.3f%s", l, H->gms[3 * l], H->gms[3 * l + 1], H->gms[3 * l + 2], l + 2 < L ? "," : "");
    printf("\n");
  }
  free(rows), free(rounds);
  return s;
}

/* The one place that makes a PCG handle for the solvers below and names its preconditioner (Jacobi: no line, the driver's or
 * sbh_solve_precond's own).  H: what pcg_levels_free releases after the handle */
static sb_pcg* build_pcg(Comm* comm, Parameter* param, void* dev_matrix, const double* b, const double* xexact, int fmt, CG_UINT C,
    CG_UINT sigma, const sbh_precond_spec* spec, pcg_levels* H)
{
  memset(H, 0, sizeof *H);
  const sb_matrix* m = (const sb_matrix*)dev_matrix;
  sb_pcg* s;
  switch (spec->kind) {
  /* the diagonal and the polynomial run on several ranks: they take the Comm's halo plan, NULL on one rank */
  case SBH_PRECOND_JACOBI: return sb_pcg_create(m, (sb_halo*)comm->dev, b, xexact, NULL);
  case SBH_PRECOND_SGS:
    s = sb_pcg_create_sgs(m, NULL, b, xexact);
    if (commIsMaster(comm)) printf("Preconditioner: SGS (multicolour symmetric Gauss-Seidel), nC = %d\n", sb_pcg_colours(s));
    return s;
  case SBH_PRECOND_POLY: {
    s = sb_pcg_create_poly(m, (sb_halo*)comm->dev, b, xexact, spec->steps ? spec->steps : 3, 0.0, 0.0);
    double iv[2];
    sb_pcg_poly_interval(s, iv);
    if (commIsMaster(comm))
      printf("Preconditioner: Chebyshev polynomial, steps = %d, lambda in [%.6g, %.6g]\n", sb_pcg_poly_steps(s), iv[0], iv[1]);
    return s;
  }
  case SBH_PRECOND_MGPOLY:
    if (spec->coarse == SBH_COARSE_AGGREGATION) return build_pcg_sa(comm, dev_matrix, sb_matrix_nr(m), b, xexact, fmt, C, sigma, spec, H);
    /* fall through */
  case SBH_PRECOND_MG:
  case SBH_PRECOND_MGFW: return build_pcg_mg(comm, param, dev_matrix, b, xexact, fmt, C, sigma, spec, H);
  }
  fprintf(stderr, "preconditioner %d: 0 jacobi, 1 sgs, 2 mg, 3 mgfw, 4 poly, 5 mgpoly\n", spec->kind);
  exit(EXIT_FAILURE);
}

/* ---- solveBiCGStab ----------------------------------------------------------------------- */
/* BiCGStab with the Jacobi right preconditioner (sb_bicgstab_*) for matrices that need not be symmetric.  The
 * lines solveCG prints while iterating are printed afterwards from the recorded r.r history: "Iteration = j" shows the
 * residual iteration j starts from, sqrt(rr[j - 1]), as solveCG and solvePCG do. */
/* solves with the handle, prints, releases it and the vectors */
static int run_bicgstab(Comm* comm, Parameter* param, sb_bicgstab* s, double* b, double* xexact)
{
  const int itermax = param->itermax, cap = itermax + 2;
  const int k    = sb_bicgstab_solve(s, itermax, param->eps);
  double* rr     = (double*)malloc((size_t)cap * sizeof(double));
  const int nRr  = sb_bicgstab_history(s, 0, rr, cap);
  print_history(comm, "", k, itermax, rr, nRr, 1);
  print_tail(comm, k, sb_bicgstab_loop_ms(s), xexact != NULL, sb_bicgstab_check_residual(s));
  sb_bicgstab_free(s);
  free(rr), free(b), free(xexact);
  return k;
}

/* ---- the one add-on solve: every sbh_solve_pcg*, sbh_solve_bicgstab* and sbh_solve_gmres* entry ------------------ */
/* PCG makes its handle with build_pcg and runs it (no spec: Jacobi).  BiCGStab and GMRES(restart) without a spec are the solvers
 * alone; with one they borrow the preconditioner plan of a PCG handle (sb_bicgstab_create_pre; sb_gmres_create_pre,
 * DESIGN 4.20), built by the same build_pcg with the same "Preconditioner: ..." line and freed after the solver.  Jacobi is a kind
 * for GMRES alone (BiCGStab's own diagonal is its default) and its line is printed here.  GMRES's printed residuals are the
 * estimates of the preconditioned operator's loop, which are those of b - A x with x = M^-1 u */
int sbh_solve_precond(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int fmt, CG_UINT C,
    CG_UINT sigma, int solver, int restart, const sbh_precond_spec* spec)
{
  static const sbh_precond_spec jacobi = { SBH_PRECOND_JACOBI, 0, 0, SBH_COARSE_REGENERATED };
  const int gmres = solver == SBH_SOLVER_GMRES, pcg = solver == SBH_SOLVER_PCG;
  const sb_matrix* m = (const sb_matrix*)dev_matrix;
  if (pcg && !spec) spec = &jacobi;
  dp_only(pcg ? "PCG: double precision only\n" : gmres ? "GMRES: double precision only\n" : "BiCGStab: double precision only\n");
  if (!pcg && spec) {
    if (comm->size > 1) mg_refuse(gmres ? "GMRES: runs on one rank" : "BiCGStab: runs on one rank");
    if (spec->kind < (gmres ? SBH_PRECOND_JACOBI : SBH_PRECOND_SGS) || spec->kind > SBH_PRECOND_MGPOLY)
      mg_refuse(gmres ? "GMRES: the preconditioners are 0 jacobi, 1 sgs, 2 mg, 3 mgfw, 4 poly, 5 mgpoly"
                      : "BiCGStab: the plan preconditioners are 1 sgs, 2 mg, 3 mgfw, 4 poly, 5 mgpoly");
  }
  double *b, *xexact;
  init_vectors_dp(param, nr, rowNnz, 1, &b, &xexact);
  if (!spec)
    return gmres ? run_gmres(comm, param, sb_gmres_create(m, NULL, b, xexact, restart), b, xexact)
                 : run_bicgstab(comm, param, sb_bicgstab_create(m, NULL, b, xexact, 1, NULL), b, xexact);
  pcg_levels H;
  sb_pcg* M = build_pcg(comm, param, dev_matrix, b, xexact, fmt, C, sigma, spec, &H);
  if (!pcg && spec->kind == SBH_PRECOND_JACOBI && commIsMaster(comm)) printf("Preconditioner: Jacobi (diagonal), nC = 0\n");
  const int k = pcg ? run_pcg(comm, param, M, b, xexact) /* (releases M) */
              : gmres ? run_gmres(comm, param, sb_gmres_create_pre(m, NULL, b, xexact, restart, M), b, xexact)
                      : run_bicgstab(comm, param, sb_bicgstab_create_pre(m, NULL, b, xexact, M), b, xexact);
  if (!pcg) sb_pcg_free(M);
  pcg_levels_free(&H);
  return k;
}

/* the entries of before: each names its solver and spec (the one-level preconditioners rebuild no matrix: no fmt, C, sigma) */
#define SPEC(...) &(const sbh_precond_spec){ __VA_ARGS__ }
int sbh_solve_pcg(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz)
{
  return sbh_solve_precond(comm, param, dev_matrix, nr, rowNnz, 0, 0, 0, SBH_SOLVER_PCG, 0, NULL);
}
int sbh_solve_pcg_sgs(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz)
{
  return sbh_solve_precond(comm, param, dev_matrix, nr, rowNnz, 0, 0, 0, SBH_SOLVER_PCG, 0, SPEC(SBH_PRECOND_SGS, 0, 0, 0));
}
int sbh_solve_pcg_poly(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int steps)
{
  return sbh_solve_precond(comm, param, dev_matrix, nr, rowNnz, 0, 0, 0, SBH_SOLVER_PCG, 0, SPEC(SBH_PRECOND_POLY, 0, steps, 0));
}
int sbh_solve_pcg_mg(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int fmt, CG_UINT C,
    CG_UINT sigma, int levels)
{
  return sbh_solve_precond(comm, param, dev_matrix, nr, rowNnz, fmt, C, sigma, SBH_SOLVER_PCG, 0, SPEC(SBH_PRECOND_MG, levels, 0, 0));
}
int sbh_solve_pcg_mgfw(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int fmt, CG_UINT C,
    CG_UINT sigma, int levels)
{
  return sbh_solve_precond(comm, param, dev_matrix, nr, rowNnz, fmt, C, sigma, SBH_SOLVER_PCG, 0, SPEC(SBH_PRECOND_MGFW, levels, 0, 0));
}
int sbh_solve_pcg_mgpoly(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int fmt, CG_UINT C,
    CG_UINT sigma, int levels, int steps)
{
  return sbh_solve_precond(comm, param, dev_matrix, nr, rowNnz, fmt, C, sigma, SBH_SOLVER_PCG, 0,
      SPEC(SBH_PRECOND_MGPOLY, levels, steps, SBH_COARSE_REGENERATED));
}
int sbh_solve_pcg_mgpoly_galerkin(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int fmt,
    CG_UINT C, CG_UINT sigma, int levels, int steps)
{
  return sbh_solve_precond(comm, param, dev_matrix, nr, rowNnz, fmt, C, sigma, SBH_SOLVER_PCG, 0,
      SPEC(SBH_PRECOND_MGPOLY, levels, steps, SBH_COARSE_GALERKIN));
}
int sbh_solve_pcg_mgpoly_sa(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int fmt, CG_UINT C,
    CG_UINT sigma, int levels, int steps)
{
  return sbh_solve_precond(comm, param, dev_matrix, nr, rowNnz, fmt, C, sigma, SBH_SOLVER_PCG, 0,
      SPEC(SBH_PRECOND_MGPOLY, levels, steps, SBH_COARSE_AGGREGATION));
}
int sbh_solve_bicgstab(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz)
{
  return sbh_solve_precond(comm, param, dev_matrix, nr, rowNnz, 0, 0, 0, SBH_SOLVER_BICGSTAB, 0, NULL);
}
int sbh_solve_bicgstab_precond(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int fmt, CG_UINT C,
    CG_UINT sigma, int precond, int levels, int steps, int galerkin)
{
  return sbh_solve_precond(comm, param, dev_matrix, nr, rowNnz, fmt, C, sigma, SBH_SOLVER_BICGSTAB, 0, SPEC(precond, levels, steps, galerkin));
}
int sbh_solve_gmres(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int restart)
{
  return sbh_solve_precond(comm, param, dev_matrix, nr, rowNnz, 0, 0, 0, SBH_SOLVER_GMRES, restart, NULL);
}
int sbh_solve_gmres_precond(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int fmt, CG_UINT C,
    CG_UINT sigma, int restart, int precond, int levels, int steps, int galerkin)
{
  return sbh_solve_precond(comm, param, dev_matrix, nr, rowNnz, fmt, C, sigma, SBH_SOLVER_GMRES, restart, SPEC(precond, levels, steps, galerkin));
}
#undef SPEC

/* ---- profiler table: src/profiler.c:11-141 ----------------------------------------------- */
static const char* const kLabel[NUMREGIONS] = { "waxpby:  ", "spMVM:   ", "ddot:    ", "comm:    " };
static double g_words[NUMREGIONS], g_flops[NUMREGIONS];

void profilerInit(size_t* facFlops, size_t* facWords)
{
  /* per-iteration work: waxpby 3 words / 6 flops per row-factor, ddot 2 / 4, spMVM words
   * given whole and 2 flops per nonzero (src/profiler.c:19-22,35-41) */
  static const double w[NUMREGIONS] = { 3, 0, 2, 0 }, fl[NUMREGIONS] = { 6, 2, 4, 0 };
  if (sb_is_initialized()) sb_region_reset();
  for (int i = 0; i < NUMREGIONS; i++) {
    _t[i]      = 0.0;
    g_words[i] = w[i] * (double)facWords[i];
    g_flops[i] = fl[i] * (double)facFlops[i];
  }
  g_words[SPMVM] = (double)facWords[SPMVM];
  g_words[COMM] = g_flops[COMM] = 0.0;
}

void profilerPrint(Comm* c, int iterations)
{
  if (!commIsMaster(c)) return;
  printf(HLINE);
  if (c->size > 1) printf("Function   Rate(MB/s)  Rate(MFlop/s)  Walltime(s)   [rank 0 of %d]\n", c->size);
  else printf("Function   Rate(MB/s)  Rate(MFlop/s)  Walltime(s)\n");
  for (int j = 0; j < NUMREGIONS - 1; j++) {
    /* a tag whose calls went through PROFILE has device-timed regions: that is the time the kernels took (the host clock in
     * _t[j] then only saw the enqueues) */
    uint64_t regions = 0;
    const double dev = sb_is_initialized() ? sb_region_seconds(j, &regions) : 0.0;
    const double t   = regions > 0 ? dev : _t[j];
    printf("%s%11.2f %11.2f %11.2f\n", kLabel[j], t > 0.0 ? 1.0E-06 * g_words[j] * iterations / t : 0.0,
        t > 0.0 ? 1.0E-06 * g_flops[j] * iterations / t : 0.0, t);
  }
  printf(HLINE);
  if (c->size > 1) {
    const double kB = 1.0E-03 * sizeof(CG_FLOAT) * (double)(c->totalSendCount + c->externalCount);
    printf("Communication (rank 0): %.2f kB per exchange, %.2e s in comm\n", kB, _t[COMM]);
    printf(HLINE);
  }
}

void profilerFinalize(void) {}
