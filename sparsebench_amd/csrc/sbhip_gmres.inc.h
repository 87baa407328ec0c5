// sbhip_gmres.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): the
// device-resident restarted GMRES(m) loop (kernels: gmres.hip.h).  Double precision, one rank.
// ===========================================================================
// GMRES
// ===========================================================================
struct sb_gmres {
  const sb_matrix* A = nullptr;
  uint32_t n = 0, nGroups = 0;
  int m = 0;
  size_t ldv = 0;
  double *V = nullptr, *w = nullptr, *r = nullptr, *x = nullptr, *b = nullptr, *Ap = nullptr, *xexact = nullptr;
  double *l1 = nullptr;       // (m + 1) * nGroups level-1 values: dot i at l1 + i * nGroups
  double *partials = nullptr; // 4 * nGroups level-0 partials (prologue, cycle close, the op list's dots)
  char* state = nullptr;      // GmScalars + the dense state of a cycle
  GmView gv;
  int hist_cap = 0;
  int fused = 1;
  int pos = 0; // cycle position of the next step (host side: only the stop flag can end a cycle early)
  LoopClock clock;
  // sb_gmres_create_pre / _dinv: GMRES on A M^-1.  x is then u, xs = M^-1 u the solution, zh = M^-1 V[j]
  RightPrecond pre; // set(): right-preconditioned
  // The polynomial's first step for V[j] is written by the step that made V[j], into the BORROWED plan's level-0 d.  Handles
  // that share the plan take turns between sb_gmres_run_steps calls, so the first step of a call at j > 0 cannot rely on d: it
  // makes that first step again from V[j] (poly_first_k: the same bits, one launch more)
  bool resumed = false;
  double *zh = nullptr, *xs = nullptr;
};

static void gm_need_vectors(const void* a, const void* b, size_t ldv, const char* fn)
{
  if ((((uintptr_t)a | (uintptr_t)b) & 15u) || (ldv & 1u)) SB_FATAL("%s: vectors must be 16-byte aligned and ldv a multiple of 2", fn);
}
// the riding mode of a test entry (sb_gmres_*_native, here and in sbhip_gmres_precond.inc.h) and the vectors it needs
static void gm_pre_native_args(int mode, const double* dinv, const double* d, const double* z, const char* fn)
{
  if (mode < -1 || mode > 1) SB_FATAL("%s: mode = %d (-1: the twin, 0: a diagonal, 1: Chebyshev)", fn, mode);
  if (mode >= 0 && (!dinv || !z || (mode == 1 && !d))) SB_FATAL("%s: mode %d needs dinv_dev, z_dev%s", fn, mode, mode ? " and d_dev" : "");
}
static dim3 gm_group_grid(uint32_t nGroups) { return dim3(stream_grid(nGroups, 4)); }
static uint32_t gm_scale_grid(uint32_t n) { return stream_grid(n, 256); }
// the step-and-normalise kernels: 1 024 threads, 4 096 rows per workgroup, at most one workgroup per CU
static uint32_t gm_step_grid(uint32_t n) { return std::max(1u, std::min((uint32_t)g.prop.multiProcessorCount, (n + 4095u) / 4096u)); }

// The three kernels that produce a vector M^-1 is applied to next, each launched as the twin f.mode picks (-1: the
// unpreconditioned kernel; 0, 1: gm_pre_*_k<mode>, which also writes pre_first<mode> of the vector to z, and d).  The loop and the
// sb_gmres_pre_*_native test entries launch them from here.
// out = a / *scalar, *g0 = *scalar
static void gm_launch_scale(uint32_t n, const double* a, const double* scalar, double* out, double* g0, const PrecondRide& f, double* z,
    const int* stop)
{
  const dim3 grid(gm_scale_grid(n)), block(256);
  if (f.mode == 1) hipLaunchKernelGGL(gm_pre_scale_k<1>, grid, block, 0, g.stream, n, a, scalar, out, g0, f.dinv, f.d, z, f.c1, stop);
  else if (f.mode == 0) hipLaunchKernelGGL(gm_pre_scale_k<0>, grid, block, 0, g.stream, n, a, scalar, out, g0, f.dinv, f.d, z, f.c1, stop);
  else hipLaunchKernelGGL(gm_scale_k, grid, block, 0, g.stream, n, a, scalar, out, g0, stop);
}
// w += c[i] * V[i], ascending i (the x update of a close)
static void gm_launch_multiadd(uint32_t n, int nvec, const double* V, size_t ldv, const double* c, double* w, const PrecondRide& f,
    double* z, const int* stop)
{
  const dim3 grid = gm_group_grid((n + 255u) >> 8), block(256);
  if (f.mode == 1) hipLaunchKernelGGL(gm_pre_multiupdate_k<1>, grid, block, 0, g.stream, n, nvec, V, ldv, c, w, f.dinv, f.d, z, f.c1, stop);
  else if (f.mode == 0) hipLaunchKernelGGL(gm_pre_multiupdate_k<0>, grid, block, 0, g.stream, n, nvec, V, ldv, c, w, f.dinv, f.d, z, f.c1, stop);
  else hipLaunchKernelGGL((gm_multiupdate_k<true, 0>), grid, block, 0, g.stream, n, nvec, V, ldv, c, w, (double*)nullptr, stop);
}
// the scalar step at cycle position j from the level-1 values of w . w, and vnext = w / hn
static void gm_launch_step(uint32_t n, const double* l1, const GmView& gv, int j, const double* w, double* vnext, const PrecondRide& f,
    double* z)
{
  const uint32_t nG = (n + 255u) >> 8;
  const dim3 grid(gm_step_grid(n)), block(1024);
  if (f.mode == 1) hipLaunchKernelGGL(gm_pre_step_k<1>, grid, block, 0, g.stream, n, nG, l1, 1, gv, j, w, vnext, f.dinv, f.d, z, f.c1);
  else if (f.mode == 0) hipLaunchKernelGGL(gm_pre_step_k<0>, grid, block, 0, g.stream, n, nG, l1, 1, gv, j, w, vnext, f.dinv, f.d, z, f.c1);
  else hipLaunchKernelGGL((gm_step_k<true>), grid, block, 0, g.stream, n, nG, l1, 1, gv, j, w, vnext);
}

// The launches the loop shares with the sb_gmres_*_native test entries, on plain pointers.
// level-1 values of dot(V[i], w), i = 0 .. nvec-1: l1[i * nGroups + group]
static void gm_launch_multidot(uint32_t n, int nvec, const double* V, size_t ldv, const double* w, double* l1, const int* stop)
{
  hipLaunchKernelGGL(gm_multidot_k, gm_group_grid((n + 255u) >> 8), dim3(256), 0, g.stream, n, nvec, V, ldv, w, l1, stop);
}
// workgroup i of nvec finishes dot i from q + i * qStride (l1 != 0: nGroups level-1 values; 0: 4 nGroups level-0 partials)
static void gm_launch_finish_dots(uint32_t nGroups, int nvec, const double* q, size_t qStride, int l1, double* out, double* nout,
    const double* add, double* sum, const int* stop)
{
  hipLaunchKernelGGL(gm_finish_dots_k, dim3(nvec), dim3(1024), 0, g.stream, nGroups, q, qStride, l1, out, nout, add, sum, stop);
}
// w -= c[i] * V[i], ascending i, and on the way out the level-1 values of the next pass's dots (epi 2) or of w . w (epi 1)
static void gm_launch_project(int epi, uint32_t n, int nvec, const double* V, size_t ldv, const double* c, double* w, double* l1,
    const int* stop)
{
  const dim3 grid = gm_group_grid((n + 255u) >> 8), block(256);
  if (epi == 2) hipLaunchKernelGGL((gm_multiupdate_k<false, 2>), grid, block, 0, g.stream, n, nvec, V, ldv, c, w, l1, stop);
  else hipLaunchKernelGGL((gm_multiupdate_k<false, 1>), grid, block, 0, g.stream, n, nvec, V, ldv, c, w, l1, stop);
}
// r.r from its partials, recorded; mode: gm_rr_k's
static void gm_launch_rr(int mode, uint32_t nGroups, const double* q, int l1, const GmView& gv, const int* stop)
{
  const dim3 grid(1), block(1024);
  if (mode == 0) hipLaunchKernelGGL((gm_rr_k<0>), grid, block, 0, g.stream, nGroups, q, l1, gv, stop);
  else if (mode == 1) hipLaunchKernelGGL((gm_rr_k<1>), grid, block, 0, g.stream, nGroups, q, l1, gv, stop);
  else hipLaunchKernelGGL((gm_rr_k<2>), grid, block, 0, g.stream, nGroups, q, l1, gv, stop);
}
static void gm_launch_backsolve(const GmView& gv, int nvec, const int* stop)
{
  hipLaunchKernelGGL(gm_backsolve_k, dim3(1), dim3(64), 0, g.stream, gv, nvec, stop);
}
// the op list's scalar step alone (one workgroup, nothing normalised)
static void gm_launch_scalar_step(uint32_t n, uint32_t nGroups, const double* q, int l1, const GmView& gv, int j)
{
  hipLaunchKernelGGL((gm_step_k<false>), dim3(1), dim3(1024), 0, g.stream, n, nGroups, q, l1, gv, j, (const double*)nullptr, (double*)nullptr);
}

// The dense state of a cycle of restart length m behind `d`, in this order: H ((m + 1) x m, column j at H + j * (m + 1)), cs, sn,
// y (m each), g, h1, h2, nh1, nh2, hcol (m + 1 each).  Returns the number of doubles.
static size_t gm_dense_layout(GmView& gv, double* d, int m)
{
  const size_t M = (size_t)m;
  double* const d0 = d;
  gv.m = m;
  gv.H = d, d += M * (M + 1);
  gv.cs = d, d += M;
  gv.sn = d, d += M;
  gv.y = d, d += M;
  gv.g = d, d += M + 1;
  gv.h1 = d, d += M + 1;
  gv.h2 = d, d += M + 1;
  gv.nh1 = d, d += M + 1;
  gv.nh2 = d, d += M + 1;
  gv.hcol = d, d += M + 1;
  return (size_t)(d - d0);
}
static size_t gm_dense_doubles(int m) { return (size_t)m * ((size_t)m + 1) + 3 * (size_t)m + 6 * ((size_t)m + 1); }
static size_t gm_state_head() { return (sizeof(GmScalars) + 15u) & ~(size_t)15u; }

// the handle behind its entry point's refusals (fn: the entry point's name in their messages)
static sb_gmres* gm_create(const sb_matrix* m, const double* b_host, const double* xexact_host, int restart, const char* fn)
{
  // the one-rank refusal in this solver's own two messages (need_one_rank has the other three's single one)
  if (multi_rank() || sb_comm_size() > 1) SB_FATAL("%s: GMRES runs on one rank (this process is rank %d of %d)", fn, g.rank, g.size);
  if (restart < 1) SB_FATAL("%s: restart = %d, expected a restart length >= 1", fn, restart);
  if (m->nc != m->nr) SB_FATAL("%s: GMRES runs on one rank: the matrix has %u halo columns", fn, m->nc - m->nr);
  sb_gmres* s = new sb_gmres();
  s->A = m, s->n = m->nr, s->m = restart;
  s->nGroups = (s->n + 255u) >> 8;
  s->ldv     = ((size_t)s->n + 511u) & ~(size_t)511u;
  if (s->ldv == 0) s->ldv = 512;
  const size_t vb = s->ldv * sizeof(double);
  s->V = (double*)sb_malloc((size_t)(restart + 1) * vb + 4096); // (the slack the CG loop's vector slab ends with: vec_layout)
  double** vecs[] = { &s->w, &s->r, &s->x, &s->b, &s->Ap };
  for (double** v : vecs) *v = (double*)sb_malloc(vb + 4096);
  upload_permuted(m, b_host, s->b);
  if (xexact_host) {
    s->xexact = (double*)sb_malloc(vb + 4096);
    upload_permuted(m, xexact_host, s->xexact);
  }
  s->l1       = (double*)sb_malloc(((size_t)(restart + 1) * s->nGroups + 4) * sizeof(double));
  s->partials = (double*)sb_malloc((4 * (size_t)s->nGroups + 4) * sizeof(double));
  HIP_CHECK(hipMemsetAsync(s->partials, 0, (4 * (size_t)s->nGroups + 4) * sizeof(double), g.stream));
  const size_t head = gm_state_head(), doubles = gm_dense_doubles(restart);
  s->state = (char*)sb_malloc(head + doubles * sizeof(double));
  HIP_CHECK(hipMemset(s->state, 0, head + doubles * sizeof(double)));
  GmView& gv = s->gv;
  gv.S = reinterpret_cast<GmScalars*>(s->state);
  gm_dense_layout(gv, reinterpret_cast<double*>(s->state + head), restart);
  gv.res_hist = gv.rr_hist = nullptr;
  s->clock.create();
  return s;
}

sb_gmres* sb_gmres_create(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int restart)
{
  need_init();
  need_dp(m, "sb_gmres_create", "GMRES");
  (void)halo;
  return gm_create(m, b_host, xexact_host, restart, "sb_gmres_create");
}

void sb_gmres_free(sb_gmres* s)
{
  if (!s) return;
  HIP_CHECK(hipStreamSynchronize(g.stream));
  s->clock.destroy();
  sb_free(s->V), sb_free(s->w), sb_free(s->r), sb_free(s->x), sb_free(s->b), sb_free(s->Ap), sb_free(s->xexact);
  sb_free(s->l1), sb_free(s->partials), sb_free(s->state), sb_free(s->gv.res_hist), sb_free(s->gv.rr_hist);
  sb_free(s->zh), sb_free(s->xs), sb_free(s->pre.dinv);
  delete s;
}

void sb_gmres_set_fused(sb_gmres* s, int fused)
{
  if (s->clock.open) SB_FATAL("sb_gmres_set_fused between sb_gmres_start and sb_gmres_finish");
  s->fused = fused ? 1 : 0;
}
int sb_gmres_restart(const sb_gmres* s) { return s->m; }

// launches of the Arnoldi step at cycle position j: SpMV | multi-dot | finish | update + pass-2 dots | finish | update + w.w |
// scalar step + normalisation = 7, + 1 at j = 0 (V[0] = r / normr) and + 5 at j = m - 1 (the cycle close: back substitution |
// x update | SpMV | r = b - A x with its r.r partials | r.r, restart).  0 for the op list.  A preconditioned handle adds A, the
// launches of an apply beyond what rides in the vector's producer, to the step and to the close.
int sb_gmres_launches_per_step(sb_gmres* s, int j)
{
  if (!s->fused) return 0;
  if (j < 0 || j >= s->m) SB_FATAL("sb_gmres_launches_per_step: cycle position %d outside 0 .. %d", j, s->m - 1);
  const int A = s->pre.apply_launches();
  return 7 + A + (j == 0 ? 1 : 0) + (j == s->m - 1 ? 5 + A : 0);
}

// r = 1.0 * b + (-1.0) * (A x) and the level-0 partials of r.r (solveCG's prologue ops, src/CGSolver.c:94-98)
static void gm_true_residual(sb_gmres* s, const int* stop)
{
  launch_spmv(s->A, s->pre.set() ? s->xs : s->x, s->Ap, nullptr, stop); // (preconditioned: x is u and xs = M^-1 u the solution)
  if (s->fused) {
    launch_dot_spans(2, s->n, s->b, s->Ap, nullptr, s->r, nullptr, s->partials, stop);
  } else {
    launch_waxpby(s->n, 1.0, s->b, -1.0, s->Ap, s->r, stop);
    launch_dot_spans(0, s->n, s->r, s->r, nullptr, nullptr, nullptr, s->partials, stop);
  }
}

// one tree dot of the op list: level-0 partials, then levels 1-2 (kernels of the parent commit's sb_ddot_async)
static void gm_op_dot(sb_gmres* s, const double* a, const double* b, double* out, double* nout, const double* add, double* sum,
    int i, const int* stop)
{
  launch_dot_spans(0, s->n, a, b, nullptr, nullptr, nullptr, s->partials, stop);
  gm_launch_finish_dots(s->nGroups, 1, s->partials, 0, 0, out + i, nout ? nout + i : nullptr, add ? add + i : nullptr, sum ? sum + i : nullptr, stop);
  HIP_CHECK(hipGetLastError());
}

// a cycle close over its nvec columns: y, x += V y (ascending), the true residual and its r.r (MODE: gm_rr_k)
template <int MODE> static void gm_close(sb_gmres* s, int nvec, const int* stop)
{
  const uint32_t n = s->n;
  gm_launch_backsolve(s->gv, nvec, stop);
  HIP_CHECK(hipGetLastError());
  const PrecondRide f = s->fused ? s->pre.ride() : PrecondRide{}; // (no preconditioner: nothing rides)
  if (n) {
    if (s->fused) gm_launch_multiadd(n, nvec, s->V, s->ldv, s->gv.y, s->x, f, s->xs, stop);
    else {
      const dim3 gridW(stream_grid(n / 2 + 1, 256)), blockW(256);
      for (int i = 0; i < nvec; i++)
        hipLaunchKernelGGL(waxpby_sdev_k, gridW, blockW, 0, g.stream, n, (const double*)s->x, (const double*)(s->gv.y + i),
            (const double*)(s->V + (size_t)i * s->ldv), s->x, stop);
    }
    HIP_CHECK(hipGetLastError());
    if (s->pre.set()) s->pre.apply(n, s->x, s->xs, stop, f.mode >= 0);
  }
  gm_true_residual(s, stop);
  gm_launch_rr(MODE, s->nGroups, s->partials, 0, s->gv, stop);
  HIP_CHECK(hipGetLastError());
}

// one Arnoldi step at cycle position j
static void gm_step(sb_gmres* s, int j)
{
  const uint32_t n = s->n, nG = s->nGroups;
  const int* stop  = &s->gv.S->stop;
  const int nvec   = j + 1;
  const GmView& gv = s->gv;
  double* Vj       = s->V + (size_t)j * s->ldv;
  double* Vn       = s->V + (size_t)(j + 1) * s->ldv;
  const PrecondRide f = s->fused && n ? s->pre.ride() : PrecondRide{}; // (no preconditioner: nothing rides)
  if (j == 0) { // V[0] = r / normr, g[0] = normr
    gm_launch_scale(n, s->r, &gv.S->normr, s->V, gv.g, f, s->zh, stop);
    HIP_CHECK(hipGetLastError());
  }
  if (s->pre.set()) { // w = A (M^-1 V[j])
    s->pre.apply(n, Vj, s->zh, stop, f.mode >= 0 && !(f.mode == 1 && s->resumed && j > 0));
    s->resumed = false;
    launch_spmv(s->A, s->zh, s->w, nullptr, stop);
  } else launch_spmv(s->A, Vj, s->w, nullptr, stop); // w = A V[j]
  if (s->fused) {
    gm_launch_multidot(n, nvec, s->V, s->ldv, s->w, s->l1, stop);
    gm_launch_finish_dots(nG, nvec, s->l1, nG, 1, gv.h1, gv.nh1, nullptr, nullptr, stop);
    gm_launch_project(2, n, nvec, s->V, s->ldv, gv.h1, s->w, s->l1, stop);
    gm_launch_finish_dots(nG, nvec, s->l1, nG, 1, gv.h2, gv.nh2, gv.h1, gv.hcol, stop);
    gm_launch_project(1, n, nvec, s->V, s->ldv, gv.h2, s->w, s->l1, stop);
    // (V[m] starts no step: at the cycle's last position nothing rides)
    gm_launch_step(n, s->l1, gv, j, s->w, Vn, j + 1 < s->m ? f : PrecondRide{}, s->zh);
    HIP_CHECK(hipGetLastError());
  } else {
    // the op list: one tree dot per h entry, one waxpby-shaped launch per projection (w = w + (-h) * V[i])
    const dim3 gridW(stream_grid(n / 2 + 1, 256)), blockW(256);
    for (int pass = 0; pass < 2; pass++) {
      double* h  = pass ? gv.h2 : gv.h1;
      double* nh = pass ? gv.nh2 : gv.nh1;
      for (int i = 0; i < nvec; i++)
        gm_op_dot(s, s->V + (size_t)i * s->ldv, s->w, h, nh, pass ? gv.h1 : nullptr, pass ? gv.hcol : nullptr, i, stop);
      for (int i = 0; i < nvec; i++)
        hipLaunchKernelGGL(waxpby_sdev_k, gridW, blockW, 0, g.stream, n, (const double*)s->w, (const double*)(nh + i),
            (const double*)(s->V + (size_t)i * s->ldv), s->w, stop);
    }
    launch_dot_spans(0, n, s->w, s->w, nullptr, nullptr, nullptr, s->partials, stop);
    gm_launch_scalar_step(n, nG, s->partials, 0, gv, j);
    gm_launch_scale(n, s->w, &gv.S->hn, Vn, nullptr, PrecondRide{}, nullptr, stop);
    HIP_CHECK(hipGetLastError());
  }
  if (j + 1 == s->m) gm_close<1>(s, s->m, stop); // a full cycle: restart from the true residual
}

void sb_gmres_start(sb_gmres* s, int itermax, double eps)
{
  need_init();
  if (s->pre.set()) need_tree("sb_gmres_start", "preconditioned GMRES", "sb_cg");
  s->pre.need_closed("sb_gmres_start");
  const int want = std::max(s->hist_cap, itermax + 2);
  grow(s->gv.res_hist, s->hist_cap, want, 1);
  grow(s->gv.rr_hist, s->hist_cap, want, 1);
  s->hist_cap = want;
  GmScalars h = zeroed<GmScalars>();
  h.eps = eps, h.itermax = itermax, h.hist_cap = s->hist_cap;
  write_block(s->gv.S, &h);
  HIP_CHECK(hipMemsetAsync(s->x, 0, s->ldv * sizeof(double), g.stream)); // x0 = 0
  if (s->pre.set()) HIP_CHECK(hipMemsetAsync(s->xs, 0, s->ldv * sizeof(double), g.stream)); // M^-1 0 = 0: the prologue needs no apply
  gm_true_residual(s, nullptr);
  gm_launch_rr(0, s->nGroups, s->partials, 0, s->gv, nullptr);
  HIP_CHECK(hipGetLastError());
  s->pos = 0;
  s->clock.begin();
}

void sb_gmres_run_steps(sb_gmres* s, int steps)
{
  need_init();
  s->clock.need_open("sb_gmres_run_steps", "sb_gmres_start");
  s->resumed = true;
  for (int i = 0; i < steps; i++) {
    gm_step(s, s->pos);
    s->pos = s->pos + 1 == s->m ? 0 : s->pos + 1;
  }
}

int sb_gmres_finish(sb_gmres* s)
{
  need_init();
  s->clock.need_open("sb_gmres_finish", "sb_gmres_start");
  s->clock.end();
  const GmScalars h = read_block(s->gv.S);
  if (h.j > 0) { // the cycle the stop flag (or the caller) left open: x takes its columns, r.r of the final x is recorded
    gm_close<2>(s, h.j, nullptr);
    HIP_CHECK(hipStreamSynchronize(g.stream));
  }
  s->clock.read();
  return h.k;
}

int sb_gmres_solve(sb_gmres* s, int itermax, double eps)
{
  sb_gmres_start(s, itermax, eps);
  sb_gmres_run_steps(s, loop_bodies(itermax));
  return sb_gmres_finish(s);
}

int sb_gmres_history(const sb_gmres* s, double* res_out, int res_cap, double* rr_out, int rr_cap, int* n_rr)
{
  need_init();
  const GmScalars h = read_block(s->gv.S);
  const int nrr     = copy_history(s->gv.rr_hist, h.n_rr, s->hist_cap, rr_out, rr_cap);
  if (n_rr) *n_rr = nrr;
  return copy_history(s->gv.res_hist, h.n_res, s->hist_cap, res_out, res_cap);
}

void sb_gmres_solution(const sb_gmres* s, double* x_host)
{
  need_init();
  download_original(s->A, s->pre.set() ? s->xs : s->x, x_host);
}

double sb_gmres_check_residual(const sb_gmres* s)
{
  need_init();
  return max_abs_diff_host(s->n, s->pre.set() ? s->xs : s->x, s->xexact);
}

double sb_gmres_loop_ms(const sb_gmres* s) { return (double)s->clock.ms; }

void sb_gmres_counters(const sb_gmres* s, int out[5])
{
  const GmScalars h = read_block(s->gv.S);
  out[0] = h.stop, out[1] = h.steps, out[2] = h.cycles, out[3] = h.n_res, out[4] = h.n_rr;
}

// grid of gm_multidot_k and gm_multiupdate_k over n rows: gm_group_grid
void sb_gmres_group_launch(uint32_t n, uint32_t out[3])
{
  need_init();
  out[0] = gm_group_grid((n + 255u) >> 8).x, out[1] = 256u, out[2] = (uint32_t)g.prop.multiProcessorCount;
}

void sb_multidot(uint32_t n, int nvec, const double* V, size_t ldv, const double* w, double* h_dev)
{
  need_init();
  if (nvec < 1 || ldv < n) SB_FATAL("sb_multidot: nvec = %d, ldv = %zu, n = %u", nvec, ldv, n);
  gm_need_vectors(V, w, ldv, "sb_multidot");
  const uint32_t nG = (n + 255u) >> 8;
  double* l1        = scratch_partials((size_t)nvec * nG + 4);
  gm_launch_multidot(n, nvec, V, ldv, w, l1, nullptr);
  gm_launch_finish_dots(nG, nvec, l1, nG, 1, h_dev, nullptr, nullptr, nullptr, nullptr);
  HIP_CHECK(hipGetLastError());
}

void sb_multiaxpy_sub(uint32_t n, int nvec, const double* V, size_t ldv, const double* h_dev, double* w)
{
  need_init();
  if (nvec < 1 || ldv < n) SB_FATAL("sb_multiaxpy_sub: nvec = %d, ldv = %zu, n = %u", nvec, ldv, n);
  gm_need_vectors(V, w, ldv, "sb_multiaxpy_sub");
  if (n == 0) return;
  hipLaunchKernelGGL((gm_multiupdate_k<false, 0>), gm_group_grid((n + 255u) >> 8), dim3(256), 0, g.stream, n, nvec, V, ldv, h_dev, w,
      (double*)nullptr, (const int*)nullptr);
  HIP_CHECK(hipGetLastError());
}

void sb_debug_sqrt_div(uint32_t n, const double* a_dev, const double* b_dev, double* sqrt_dev, double* div_dev)
{
  need_init();
  if (n == 0) return;
  hipLaunchKernelGGL(gm_sqrt_div_k, dim3(stream_grid(n, 256)), dim3(256), 0, g.stream, n, a_dev, b_dev, sqrt_dev, div_dev);
  HIP_CHECK(hipGetLastError());
}

// --- blocking test entries: every kernel of the loop alone, launched by the loop's own gm_launch_* functions ---------------------
// grid of gm_scale_k / gm_pre_scale_k and of gm_step_k<true> / gm_pre_step_k over n rows: {workgroups, threads, CUs}
void sb_gmres_scale_launch(uint32_t n, uint32_t out[3])
{
  need_init();
  out[0] = gm_scale_grid(n), out[1] = 256u, out[2] = (uint32_t)g.prop.multiProcessorCount;
}
void sb_gmres_step_launch(uint32_t n, uint32_t out[3])
{
  need_init();
  out[0] = gm_step_grid(n), out[1] = 1024u, out[2] = (uint32_t)g.prop.multiProcessorCount;
}

// The state block of a test entry: the caller's plain data (include/sbhip.h: blk_d[4], blk_i[9] in GmScalars' order, then the
// dense state of restart length m in gm_dense_layout's order) uploaded between two runs of guard words as gm_create lays it out,
// downloaded again behind the launch.  Nothing in between is computed here.
namespace {
enum { GM_BLK_GUARD = 64 }; // guard words (8 bytes each) in front of the block and behind the dense state
struct GmTestState {
  std::vector<unsigned long long> up;
  char* raw = nullptr;
  GmView gv;
  size_t dense = 0; // doubles of the dense state (0: the block alone)
  static size_t head_words() { return gm_state_head() / 8; }
  GmTestState(const double* d, const int* i, int m, const double* dense_host, double* res_hist_dev, double* rr_hist_dev)
  {
    static_assert(sizeof(GmScalars) % 8 == 0, "the block is a whole number of guard-sized words");
    GmScalars h = zeroed<GmScalars>();
    h.normr = d[0], h.eps = d[1], h.hn = d[2], h.rr = d[3];
    h.stop = i[0], h.k = i[1], h.j = i[2], h.itermax = i[3], h.n_res = i[4], h.n_rr = i[5], h.hist_cap = i[6], h.cycles = i[7], h.steps = i[8];
    dense = dense_host ? gm_dense_doubles(m) : 0;
    up.resize(2 * GM_BLK_GUARD + head_words() + dense);
    for (size_t k = 0; k < up.size(); k++) up[k] = 0x7FF8C0DE00000000ull | k; // quiet NaNs with a payload
    memcpy(&up[GM_BLK_GUARD], &h, sizeof h);
    if (dense) memcpy(&up[GM_BLK_GUARD + head_words()], dense_host, dense * 8);
    raw = (char*)sb_malloc(up.size() * 8);
    HIP_CHECK(hipStreamSynchronize(g.stream));
    HIP_CHECK(hipMemcpy(raw, up.data(), up.size() * 8, hipMemcpyHostToDevice));
    memset(&gv, 0, sizeof gv);
    gv.S = reinterpret_cast<GmScalars*>(raw + 8 * GM_BLK_GUARD);
    gv.m = m;
    if (dense) gm_dense_layout(gv, reinterpret_cast<double*>(raw + 8 * (GM_BLK_GUARD + head_words())), m);
    gv.res_hist = res_hist_dev, gv.rr_hist = rr_hist_dev;
  }
  const int* stop() const { return &gv.S->stop; }
  // waits for the launch; the block and the dense state back to the caller; returns the number of guard words that changed (the
  // words between the block and the dense state are guards too)
  int done(double* d, int* i, double* dense_host)
  {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(g.stream));
    std::vector<unsigned long long> back(up.size());
    HIP_CHECK(hipMemcpy(back.data(), raw, back.size() * 8, hipMemcpyDeviceToHost));
    sb_free(raw);
    const size_t blk0 = GM_BLK_GUARD, blk1 = blk0 + sizeof(GmScalars) / 8, dense0 = blk0 + head_words(), dense1 = dense0 + dense;
    int changed = 0;
    for (size_t k = 0; k < back.size(); k++)
      if ((k < blk0 || (k >= blk1 && k < dense0) || k >= dense1) && back[k] != up[k]) changed++;
    GmScalars h;
    memcpy(&h, &back[blk0], sizeof h);
    d[0] = h.normr, d[1] = h.eps, d[2] = h.hn, d[3] = h.rr;
    i[0] = h.stop, i[1] = h.k, i[2] = h.j, i[3] = h.itermax, i[4] = h.n_res, i[5] = h.n_rr, i[6] = h.hist_cap, i[7] = h.cycles, i[8] = h.steps;
    if (dense) memcpy(dense_host, &back[dense0], dense * 8);
    return changed;
  }
};
// a stop flag alone (the kernels that read one and no other field): a block whose only set field is `stop`; done() also counts a
// changed block
struct GmTestFlag {
  double d[4] = { 0.0, 0.0, 0.0, 0.0 };
  int i[9]    = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
  int stopped;
  GmTestState st;
  static const int* first(int* i, int stopped) { return i[0] = stopped ? 1 : 0, i; }
  explicit GmTestFlag(int stopped_) : stopped(stopped_ ? 1 : 0), st(d, first(i, stopped_), 0, nullptr, nullptr, nullptr) {}
  const int* stop() const { return st.stop(); }
  int done()
  {
    int changed = st.done(d, i, nullptr);
    for (int k = 0; k < 4; k++) changed += d[k] != 0.0;
    for (int k = 0; k < 9; k++) changed += i[k] != (k == 0 ? stopped : 0);
    return changed;
  }
};
} // namespace

// level-1 values of dot(V[i], w) into l1_dev[i * nGroups + group], nGroups = (n + 255) / 256
int sb_gmres_multidot_native(uint32_t n, int nvec, const double* V_dev, size_t ldv, const double* w_dev, double* l1_dev, int stopped)
{
  need_init();
  if (nvec < 1 || ldv < n) SB_FATAL("sb_gmres_multidot_native: nvec = %d, ldv = %zu, n = %u", nvec, ldv, n);
  gm_need_vectors(V_dev, w_dev, ldv, "sb_gmres_multidot_native");
  GmTestFlag f(stopped);
  gm_launch_multidot(n, nvec, V_dev, ldv, w_dev, l1_dev, f.stop());
  return f.done();
}

// gm_finish_dots_k on nvec workgroups; nout_dev, add_dev / sum_dev may be NULL (sum_dev needs add_dev)
int sb_gmres_finish_dots_native(uint32_t nGroups, int nvec, const double* q_dev, size_t qStride, int l1, double* out_dev, double* nout_dev,
    const double* add_dev, double* sum_dev, int stopped)
{
  need_init();
  if (nvec < 1 || (sum_dev && !add_dev)) SB_FATAL("sb_gmres_finish_dots_native: nvec = %d%s", nvec, sum_dev && !add_dev ? ", sum_dev without add_dev" : "");
  need_aligned16({ q_dev }, "sb_gmres_finish_dots_native", "partials");
  if (qStride & 1u) SB_FATAL("sb_gmres_finish_dots_native: qStride = %zu, expected a multiple of 2", qStride);
  GmTestFlag f(stopped);
  gm_launch_finish_dots(nGroups, nvec, q_dev, qStride, l1, out_dev, nout_dev, add_dev, sum_dev, f.stop());
  return f.done();
}

// gm_multiupdate_k<false, epi>, epi 1 or 2: w -= c[i] * V[i] and the level-1 values of w . w into l1_dev[group] (1) or of
// dot(V[i], w) into l1_dev[i * nGroups + group] (2)
int sb_gmres_project_native(int epi, uint32_t n, int nvec, const double* V_dev, size_t ldv, const double* c_dev, double* w_dev, double* l1_dev,
    int stopped)
{
  need_init();
  if (epi != 1 && epi != 2) SB_FATAL("sb_gmres_project_native: epi = %d, expected 1 or 2 (0 is sb_multiaxpy_sub)", epi);
  if (nvec < 1 || ldv < n) SB_FATAL("sb_gmres_project_native: nvec = %d, ldv = %zu, n = %u", nvec, ldv, n);
  gm_need_vectors(V_dev, w_dev, ldv, "sb_gmres_project_native");
  GmTestFlag f(stopped);
  if (n) gm_launch_project(epi, n, nvec, V_dev, ldv, c_dev, w_dev, l1_dev, f.stop());
  return f.done();
}

// gm_multiupdate_k<true, 0> (mode -1) and gm_pre_multiupdate_k<mode>: sb_gmres_pre_multiupdate_native with a stop flag
int sb_gmres_multiadd_native(uint32_t n, int mode, double c1, int nvec, const double* V_dev, size_t ldv, const double* c_dev, double* w_dev,
    const double* dinv_dev, double* d_dev, double* z_dev, int stopped)
{
  need_init();
  gm_pre_native_args(mode, dinv_dev, d_dev, z_dev, "sb_gmres_multiadd_native");
  if (nvec < 1 || ldv < n) SB_FATAL("sb_gmres_multiadd_native: nvec = %d, ldv = %zu, n = %u", nvec, ldv, n);
  gm_need_vectors(V_dev, w_dev, ldv, "sb_gmres_multiadd_native");
  if (mode >= 0) need_aligned16({ dinv_dev, d_dev, z_dev }, "sb_gmres_multiadd_native", "vectors");
  GmTestFlag f(stopped);
  if (n) gm_launch_multiadd(n, nvec, V_dev, ldv, c_dev, w_dev, PrecondRide{ mode, dinv_dev, d_dev, c1 }, z_dev, f.stop());
  return f.done();
}

// gm_scale_k (mode -1) and gm_pre_scale_k<mode>: sb_gmres_pre_scale_native with a stop flag; g0_dev may be NULL
int sb_gmres_scale_native(uint32_t n, int mode, double c1, const double* a_dev, const double* scalar_dev, double* out_dev, double* g0_dev,
    const double* dinv_dev, double* d_dev, double* z_dev, int stopped)
{
  need_init();
  gm_pre_native_args(mode, dinv_dev, d_dev, z_dev, "sb_gmres_scale_native");
  GmTestFlag f(stopped);
  if (n) gm_launch_scale(n, a_dev, scalar_dev, out_dev, g0_dev, PrecondRide{ mode, dinv_dev, d_dev, c1 }, z_dev, f.stop());
  return f.done();
}

// gm_rr_k<mode> on the caller's block and histories (hist_cap entries each); use_stop: the launch is handed the block's flag (the
// close inside the loop) or none (the prologue, and the close sb_gmres_finish makes)
int sb_gmres_rr_native(int mode, uint32_t nGroups, const double* q_dev, int l1, double* res_hist_dev, double* rr_hist_dev, int use_stop,
    double* blk_d, int* blk_i)
{
  need_init();
  if (mode < 0 || mode > 2) SB_FATAL("sb_gmres_rr_native: mode = %d outside 0 .. 2", mode);
  need_aligned16({ q_dev }, "sb_gmres_rr_native", "partials");
  GmTestState st(blk_d, blk_i, 0, nullptr, res_hist_dev, rr_hist_dev);
  gm_launch_rr(mode, nGroups, q_dev, l1, st.gv, use_stop ? st.stop() : nullptr);
  return st.done(blk_d, blk_i, nullptr);
}

// The scalar step at cycle position j of a cycle of restart length m on the caller's block, dense state and res_hist.
// scale 0: gm_step_k<false> over nGroups values at q_dev (l1 != 0: level-1 values, 0: 4 nGroups level-0 partials); nothing else
// is read.  scale 1: gm_step_k<true> (mode -1) or gm_pre_step_k<mode>: q_dev holds the (n + 255) / 256 level-1 values of w . w
// (nGroups and l1 are not read), vnext = w / hn and the first part of M^-1 of it.  The kernel reads the block's own stop flag.
int sb_gmres_step_native(int scale, int mode, double c1, uint32_t n, int j, int m, uint32_t nGroups, const double* q_dev, int l1,
    const double* w_dev, double* vnext_dev, const double* dinv_dev, double* d_dev, double* z_dev, double* res_hist_dev, double* blk_d, int* blk_i,
    double* dense_host)
{
  need_init();
  if (m < 1 || m > 1024 || j < 0 || j >= m) SB_FATAL("sb_gmres_step_native: cycle position %d of restart length %d", j, m);
  if (!dense_host) SB_FATAL("sb_gmres_step_native: no dense_host");
  need_aligned16({ q_dev }, "sb_gmres_step_native", "partials");
  if (scale) gm_pre_native_args(mode, dinv_dev, d_dev, z_dev, "sb_gmres_step_native");
  else if (mode != -1) SB_FATAL("sb_gmres_step_native: scale 0 takes mode -1 only (mode = %d)", mode);
  GmTestState st(blk_d, blk_i, m, dense_host, res_hist_dev, nullptr);
  if (scale) gm_launch_step(n, q_dev, st.gv, j, w_dev, vnext_dev, PrecondRide{ mode, dinv_dev, d_dev, c1 }, z_dev);
  else gm_launch_scalar_step(n, nGroups, q_dev, l1, st.gv, j);
  return st.done(blk_d, blk_i, dense_host);
}

// gm_backsolve_k over the first nvec columns of the caller's dense state of restart length m; use_stop as in sb_gmres_rr_native
int sb_gmres_backsolve_native(int m, int nvec, int use_stop, double* blk_d, int* blk_i, double* dense_host)
{
  need_init();
  if (m < 1 || m > 1024 || nvec < 0 || nvec > m) SB_FATAL("sb_gmres_backsolve_native: %d columns of restart length %d", nvec, m);
  if (!dense_host) SB_FATAL("sb_gmres_backsolve_native: no dense_host");
  GmTestState st(blk_d, blk_i, m, dense_host, nullptr, nullptr);
  gm_launch_backsolve(st.gv, nvec, use_stop ? st.stop() : nullptr);
  return st.done(blk_d, blk_i, dense_host);
}
