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
static dim3 gm_group_grid(uint32_t nGroups) { return dim3(stream_grid(nGroups, 4)); }

// The three kernels that produce a vector M^-1 is applied to next, each launched as the twin f.mode picks (-1: the
// unpreconditioned kernel; 0, 1: gm_pre_*_k<mode>, which also writes pre_first<mode> of the vector to z, and d).  The loop and the
// sb_gmres_pre_*_native test entries launch them from here.
// out = a / *scalar, *g0 = *scalar
static void gm_launch_scale(uint32_t n, const double* a, const double* scalar, double* out, double* g0, const PrecondRide& f, double* z,
    const int* stop)
{
  const dim3 grid(stream_grid(n, 256)), block(256);
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
  const dim3 grid(std::max(1u, std::min((uint32_t)g.prop.multiProcessorCount, (n + 4095u) / 4096u))), block(1024);
  if (f.mode == 1) hipLaunchKernelGGL(gm_pre_step_k<1>, grid, block, 0, g.stream, n, nG, l1, 1, gv, j, w, vnext, f.dinv, f.d, z, f.c1);
  else if (f.mode == 0) hipLaunchKernelGGL(gm_pre_step_k<0>, grid, block, 0, g.stream, n, nG, l1, 1, gv, j, w, vnext, f.dinv, f.d, z, f.c1);
  else hipLaunchKernelGGL((gm_step_k<true>), grid, block, 0, g.stream, n, nG, l1, 1, gv, j, w, vnext);
}

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
  const size_t M = (size_t)restart, head = (sizeof(GmScalars) + 15u) & ~(size_t)15u;
  const size_t doubles = M * (M + 1) + 3 * M + 6 * (M + 1);
  s->state = (char*)sb_malloc(head + doubles * sizeof(double));
  HIP_CHECK(hipMemset(s->state, 0, head + doubles * sizeof(double)));
  double* d = reinterpret_cast<double*>(s->state + head);
  GmView& gv = s->gv;
  gv.S = reinterpret_cast<GmScalars*>(s->state), gv.m = restart;
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
  hipLaunchKernelGGL(gm_finish_dots_k, dim3(1), dim3(1024), 0, g.stream, s->nGroups, (const double*)s->partials, (size_t)0, 0,
      out + i, nout ? nout + i : nullptr, add ? add + i : nullptr, sum ? sum + i : nullptr, stop);
  HIP_CHECK(hipGetLastError());
}

// a cycle close over its nvec columns: y, x += V y (ascending), the true residual and its r.r (MODE: gm_rr_k)
template <int MODE> static void gm_close(sb_gmres* s, int nvec, const int* stop)
{
  const uint32_t n = s->n;
  hipLaunchKernelGGL(gm_backsolve_k, dim3(1), dim3(64), 0, g.stream, s->gv, nvec, stop);
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
  hipLaunchKernelGGL((gm_rr_k<MODE>), dim3(1), dim3(1024), 0, g.stream, s->nGroups, (const double*)s->partials, 0, s->gv, stop);
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
    const dim3 gridG = gm_group_grid(nG), gridD(nvec);
    hipLaunchKernelGGL(gm_multidot_k, gridG, dim3(256), 0, g.stream, n, nvec, (const double*)s->V, s->ldv, (const double*)s->w, s->l1, stop);
    hipLaunchKernelGGL(gm_finish_dots_k, gridD, dim3(1024), 0, g.stream, nG, (const double*)s->l1, (size_t)nG, 1, gv.h1, gv.nh1,
        (const double*)nullptr, (double*)nullptr, stop);
    hipLaunchKernelGGL((gm_multiupdate_k<false, 2>), gridG, dim3(256), 0, g.stream, n, nvec, (const double*)s->V, s->ldv,
        (const double*)gv.h1, s->w, s->l1, stop);
    hipLaunchKernelGGL(gm_finish_dots_k, gridD, dim3(1024), 0, g.stream, nG, (const double*)s->l1, (size_t)nG, 1, gv.h2, gv.nh2,
        (const double*)gv.h1, gv.hcol, stop);
    hipLaunchKernelGGL((gm_multiupdate_k<false, 1>), gridG, dim3(256), 0, g.stream, n, nvec, (const double*)s->V, s->ldv,
        (const double*)gv.h2, s->w, s->l1, stop);
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
    hipLaunchKernelGGL((gm_step_k<false>), dim3(1), dim3(1024), 0, g.stream, n, nG, (const double*)s->partials, 0, gv, j,
        (const double*)nullptr, (double*)nullptr);
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
  hipLaunchKernelGGL((gm_rr_k<0>), dim3(1), dim3(1024), 0, g.stream, s->nGroups, (const double*)s->partials, 0, s->gv, (const int*)nullptr);
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
  hipLaunchKernelGGL(gm_multidot_k, gm_group_grid(nG), dim3(256), 0, g.stream, n, nvec, V, ldv, w, l1, (const int*)nullptr);
  hipLaunchKernelGGL(gm_finish_dots_k, dim3(nvec), dim3(1024), 0, g.stream, nG, (const double*)l1, (size_t)nG, 1, h_dev, (double*)nullptr,
      (const double*)nullptr, (double*)nullptr, (const int*)nullptr);
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
