// sbhip_bicgstab.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context):
// right-preconditioned BiCGStab with a diagonal preconditioner (kernels: bicgstab.hip.h), or with the preconditioner
// plan of a borrowed sb_pcg handle (ph = V(0, p), sh = V(0, s) by precond_cycle).  Double precision, one
// rank, tree dot order.  The SpMV is the one the matrix's kernel mode selects (launch_spmv: the reference-layout stream or the
// masked row programs), WITHOUT a fused dot: neither rhat.v nor t.s is x.y of its SpMV.  The loop's vectors are allocations of
// the handle's own: the matrix's tuned arena (sb_matrix::vecArena) is laid out for sb_cg's vectors and stays with sb_cg.
// ===========================================================================
// BiCGStab
// ===========================================================================
struct sb_bicgstab {
  const sb_matrix* A = nullptr;
  uint32_t nr = 0, nc = 0, nGroups = 0;
  // device row order; s lives in r's storage
  double *r = nullptr, *rhat = nullptr, *p = nullptr, *ph = nullptr, *v = nullptr, *sh = nullptr, *t = nullptr, *x = nullptr, *b = nullptr;
  double* xexact = nullptr;
  BicgScalars* S = nullptr;
  double *l1a = nullptr, *l1b = nullptr;
  double* hist = nullptr; // 5 x hist_cap: rr, rho, rv, ts, tt
  int hist_cap = 0;
  int k_next = 1;
  LoopClock clock;
  RightPrecond pre; // the handle's own diagonal, or (sb_bicgstab_create_pre) the plan of a borrowed PCG handle
};

// grid of the four streaming kernels over n rows: vec_stream_grid
void sb_bicgstab_launch(uint32_t n, uint32_t out[3])
{
  need_init();
  out[0] = vec_stream_grid(n), out[1] = 1024u, out[2] = (uint32_t)g.prop.multiProcessorCount;
}

// the control block of a blocking test entry: its three coefficients, everything else zero
static BicgScalars* bicg_coeffs(double alpha, double omega, double beta)
{
  BicgScalars h = zeroed<BicgScalars>();
  h.alpha = alpha, h.omega = omega, h.beta = beta;
  return test_block(h);
}

// the p update (the s update below) whose kernel f.mode picks: -1 bicg_plan_update_p_k<0>, 0 bicg_update_p_k, 1
// bicg_plan_update_p_k<1>
static void bicg_launch_update_p(uint32_t n, const double* r, double* p, const double* v, const PrecondRide& f, double* ph,
    const BicgScalars* S)
{
  const dim3 grid(vec_stream_grid(n)), block(1024);
  if (f.mode == 1) hipLaunchKernelGGL(bicg_plan_update_p_k<1>, grid, block, 0, g.stream, n, r, p, v, f.dinv, f.d, ph, f.c1, S);
  else if (f.mode == 0) hipLaunchKernelGGL(bicg_update_p_k, grid, block, 0, g.stream, n, r, p, v, f.dinv, ph, S);
  else hipLaunchKernelGGL(bicg_plan_update_p_k<0>, grid, block, 0, g.stream, n, r, p, v, f.dinv, f.d, (double*)nullptr, f.c1, S);
}
static void bicg_launch_update_s(uint32_t n, const double* r, const double* v, double* s, const PrecondRide& f, double* sh,
    const BicgScalars* S)
{
  const dim3 grid(vec_stream_grid(n)), block(1024);
  if (f.mode == 1) hipLaunchKernelGGL(bicg_plan_update_s_k<1>, grid, block, 0, g.stream, n, r, v, f.dinv, s, f.d, sh, f.c1, S);
  else if (f.mode == 0) hipLaunchKernelGGL(bicg_update_s_k, grid, block, 0, g.stream, n, r, v, f.dinv, s, sh, S);
  else hipLaunchKernelGGL(bicg_plan_update_s_k<0>, grid, block, 0, g.stream, n, r, v, f.dinv, s, f.d, (double*)nullptr, f.c1, S);
}

void sb_bicgstab_update_p_native(uint32_t n, double beta, double omega, const double* r_dev, double* p_dev, const double* v_dev,
    const double* dinv_dev, double* ph_dev)
{
  need_init();
  if (n == 0) return;
  need_aligned16({ r_dev, p_dev, v_dev, dinv_dev, ph_dev }, "sb_bicgstab_update_p_native", "vectors");
  BicgScalars* S = bicg_coeffs(0.0, omega, beta);
  bicg_launch_update_p(n, r_dev, p_dev, v_dev, PrecondRide{ 0, dinv_dev }, ph_dev, S);
  test_block_done(S);
}

void sb_bicgstab_update_s_native(uint32_t n, double alpha, const double* r_dev, const double* v_dev, const double* dinv_dev, double* s_dev,
    double* sh_dev)
{
  need_init();
  if (n == 0) return;
  need_aligned16({ r_dev, v_dev, dinv_dev, s_dev, sh_dev }, "sb_bicgstab_update_s_native", "vectors");
  BicgScalars* S = bicg_coeffs(alpha, 0.0, 0.0);
  bicg_launch_update_s(n, r_dev, v_dev, s_dev, PrecondRide{ 0, dinv_dev }, sh_dev, S);
  test_block_done(S);
}

// cheb 0: p alone (dinv, d, ph unused, may be NULL); cheb 1: with d = (p o dinv) * c1 and ph = d
void sb_bicgstab_plan_update_p_native(uint32_t n, int cheb, double c1, double beta, double omega, const double* r_dev, double* p_dev,
    const double* v_dev, const double* dinv_dev, double* d_dev, double* ph_dev)
{
  need_init();
  if (n == 0) return;
  need_aligned16({ r_dev, p_dev, v_dev }, "sb_bicgstab_plan_update_p_native", "vectors");
  if (cheb) need_aligned16({ dinv_dev, d_dev, ph_dev }, "sb_bicgstab_plan_update_p_native", "vectors");
  if (cheb && (!dinv_dev || !d_dev || !ph_dev)) SB_FATAL("sb_bicgstab_plan_update_p_native: cheb = 1 needs dinv_dev, d_dev and ph_dev");
  BicgScalars* S = bicg_coeffs(0.0, omega, beta);
  bicg_launch_update_p(n, r_dev, p_dev, v_dev, cheb ? PrecondRide{ 1, dinv_dev, d_dev, c1 } : PrecondRide{}, ph_dev, S);
  test_block_done(S);
}

void sb_bicgstab_plan_update_s_native(uint32_t n, int cheb, double c1, double alpha, const double* r_dev, const double* v_dev,
    const double* dinv_dev, double* s_dev, double* d_dev, double* sh_dev)
{
  need_init();
  if (n == 0) return;
  need_aligned16({ r_dev, v_dev, s_dev }, "sb_bicgstab_plan_update_s_native", "vectors");
  if (cheb) need_aligned16({ dinv_dev, d_dev, sh_dev }, "sb_bicgstab_plan_update_s_native", "vectors");
  if (cheb && (!dinv_dev || !d_dev || !sh_dev)) SB_FATAL("sb_bicgstab_plan_update_s_native: cheb = 1 needs dinv_dev, d_dev and sh_dev");
  BicgScalars* S = bicg_coeffs(alpha, 0.0, 0.0);
  bicg_launch_update_s(n, r_dev, v_dev, s_dev, cheb ? PrecondRide{ 1, dinv_dev, d_dev, c1 } : PrecondRide{}, sh_dev, S);
  test_block_done(S);
}

void sb_bicgstab_dot2_native(uint32_t n, int pair, const double* a_dev, const double* b_dev, double* l1_ab_dev, double* l1_aa_dev)
{
  need_init();
  if (n == 0) return;
  need_aligned16({ a_dev, b_dev }, "sb_bicgstab_dot2_native", "vectors");
  if (pair)
    hipLaunchKernelGGL(bicg_dot2_k, dim3(vec_stream_grid(n)), dim3(1024), 0, g.stream, n, a_dev, b_dev, l1_ab_dev, l1_aa_dev, (const int*)nullptr);
  else
    hipLaunchKernelGGL(dot_l1_k, dim3(vec_stream_grid(n)), dim3(1024), 0, g.stream, n, a_dev, b_dev, l1_ab_dev, (const int*)nullptr);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(g.stream));
}

void sb_bicgstab_update_xr_native(uint32_t n, double alpha, double omega, double* x_dev, const double* ph_dev, const double* sh_dev,
    const double* s_dev, const double* t_dev, const double* rhat_dev, double* r_dev, double* l1_rho_dev, double* l1_rr_dev)
{
  need_init();
  if (n == 0) return;
  need_aligned16({ x_dev, ph_dev, sh_dev, s_dev, t_dev, rhat_dev, r_dev }, "sb_bicgstab_update_xr_native", "vectors");
  BicgScalars* S = bicg_coeffs(alpha, omega, 0.0);
  hipLaunchKernelGGL(bicg_update_xr_k, dim3(vec_stream_grid(n)), dim3(1024), 0, g.stream, n, x_dev, ph_dev, sh_dev, s_dev, t_dev, rhat_dev, r_dev,
      (const BicgScalars*)S, l1_rho_dev, l1_rr_dev);
  test_block_done(S);
}

// the scalar step's reduction alone: the totals of two arrays of m level-1 values, as the prologue step forms them
void sb_bicgstab_reduce_native(uint32_t m, const double* l1_a_dev, const double* l1_b_dev, double out[2])
{
  need_init();
  BicgScalars* S = bicg_coeffs(0.0, 0.0, 0.0); // itermax = 0, hist_cap = 0: nothing is recorded
  hipLaunchKernelGGL((bicg_scalar_k<0>), dim3(1), dim3(1024), 0, g.stream, m, l1_a_dev, l1_b_dev, S, (double*)nullptr);
  HIP_CHECK(hipGetLastError());
  const BicgScalars h = read_block(S);
  sb_free(S);
  out[0] = h.rho, out[1] = h.rr;
}

// the handle and its loop vectors
static size_t bicg_vector_bytes(const sb_matrix* m) { return (size_t)m->nc * sizeof(double) + 4096; }
static sb_bicgstab* bicg_alloc(const sb_matrix* m)
{
  sb_bicgstab* s  = new sb_bicgstab();
  s->A = m, s->nr = m->nr, s->nc = m->nc;
  s->nGroups      = (m->nr + 255u) >> 8;
  double** vecs[] = { &s->r, &s->rhat, &s->p, &s->ph, &s->v, &s->sh, &s->t, &s->x, &s->b };
  for (double** vv : vecs) *vv = (double*)sb_malloc(bicg_vector_bytes(m));
  return s;
}
// b, the exact solution, the control block and the level-1 arrays
static void bicg_finish_create(sb_bicgstab* s, const double* b_host, const double* xexact_host)
{
  const sb_matrix* m = s->A;
  upload_permuted(m, b_host, s->b);
  if (xexact_host) {
    s->xexact = (double*)sb_malloc((size_t)m->nr * sizeof(double) + 4096);
    upload_permuted(m, xexact_host, s->xexact);
  }
  s->S = (BicgScalars*)sb_malloc(sizeof(BicgScalars));
  HIP_CHECK(hipMemset(s->S, 0, sizeof(BicgScalars)));
  const size_t lb = ((size_t)s->nGroups + 4) * sizeof(double);
  double** l1s[]  = { &s->l1a, &s->l1b };
  for (double** vv : l1s) {
    *vv = (double*)sb_malloc(lb);
    HIP_CHECK(hipMemsetAsync(*vv, 0, lb, g.stream));
  }
  s->clock.create();
  HIP_CHECK(hipStreamSynchronize(g.stream));
}

sb_bicgstab* sb_bicgstab_create(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int precond,
    const double* dinv_host)
{
  need_init();
  need_dp(m, "sb_bicgstab_create", "BiCGStab");
  need_one_rank(m, halo, "sb_bicgstab_create", "BiCGStab");
  need_tree("sb_bicgstab_create", "BiCGStab", "sb_cg");
  if (precond < 0 || precond > 2) SB_FATAL("sb_bicgstab_create: precond = %d (0: none, 1: Jacobi, 2: the caller's dinv_host)", precond);
  if (precond == 2) {
    if (!dinv_host) SB_FATAL("sb_bicgstab_create: precond = 2 needs dinv_host");
    for (uint32_t i = 0; i < m->nr; i++)
      if (!(dinv_host[i] != 0.0 && fabs(dinv_host[i]) < INFINITY))
        SB_FATAL("sb_bicgstab_create: dinv[%u] = %g: the preconditioner's entries must be finite and non-zero", i, dinv_host[i]);
  }
  const size_t nb = (size_t)m->nr * sizeof(double);
  std::vector<double> hd; // the preconditioner on the host: original order (none, the caller's) or device order (Jacobi)
  double* tmp = scratch_ws(0, (size_t)m->nr + 2);
  if (precond == 1 && m->nr) { // Jacobi: dinv = 1 / diag(A), d by sb_matrix_diagonal's rule.  Checked on the host, for finite and
                               // NON-ZERO (PCG's check is for finite and positive, inside diag_*_k: the two stay apart)
    hd.resize(m->nr);
    launch_diagonal(m, tmp, nullptr);
    sb_d2h(hd.data(), tmp, nb);
    uint32_t bad = 0, first = 0;
    for (uint32_t i = 0; i < m->nr; i++)
      if (!(hd[i] != 0.0 && fabs(hd[i]) < INFINITY)) {
        if (!bad) first = i;
        bad++;
      }
    if (bad)
      SB_FATAL("sb_bicgstab_create: %u of %u matrix rows have no finite non-zero diagonal entry (the first: device row %u): the "
               "Jacobi preconditioner needs one in every row; pass precond 0 or a dinv_host of your own", bad, m->nr, first);
  }
  sb_bicgstab* s = bicg_alloc(m);
  s->pre.dinv    = (double*)sb_malloc(bicg_vector_bytes(m));
  if (precond != 1) {
    if (precond == 0) hd.assign(m->nr, 1.0);
    upload_permuted(m, precond == 0 ? hd.data() : dinv_host, s->pre.dinv);
  } else if (m->nr) {
    hipLaunchKernelGGL(pcg_reciprocal_k, dim3(stream_grid(m->nr, 256)), dim3(256), 0, g.stream, m->nr, (const double*)tmp, s->pre.dinv);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(g.stream));
  }
  bicg_finish_create(s, b_host, xexact_host);
  return s;
}

// M's preconditioner in the diagonal's place.  M is borrowed (RightPrecond): it must outlive the handle, be made over the same
// matrix, and have no solve open here or at any sb_bicgstab_start.  A plan-less M: its dinv is copied, the handle is a diagonal one
sb_bicgstab* sb_bicgstab_create_pre(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, const sb_pcg* M)
{
  need_init();
  need_dp(m, "sb_bicgstab_create_pre", "BiCGStab");
  need_one_rank(m, halo, "sb_bicgstab_create_pre", "BiCGStab");
  need_tree("sb_bicgstab_create_pre", "BiCGStab", "sb_cg");
  RightPrecond::need_borrowable(m, M, "sb_bicgstab_create_pre");
  sb_bicgstab* s = bicg_alloc(m);
  s->pre.borrow(M, bicg_vector_bytes(m));
  bicg_finish_create(s, b_host, xexact_host);
  return s;
}

// 0: a diagonal; else the plan's kind as sb_pcg_precond reports it
int sb_bicgstab_precond(const sb_bicgstab* s) { return s->pre.kind(); }

void sb_bicgstab_free(sb_bicgstab* s)
{
  if (!s) return;
  HIP_CHECK(hipStreamSynchronize(g.stream));
  s->clock.destroy();
  sb_free(s->r), sb_free(s->rhat), sb_free(s->p), sb_free(s->ph), sb_free(s->v), sb_free(s->sh), sb_free(s->t), sb_free(s->x);
  sb_free(s->b), sb_free(s->pre.dinv), sb_free(s->xexact), sb_free(s->S), sb_free(s->l1a), sb_free(s->l1b), sb_free(s->hist);
  delete s;
}

// launches per loop body: p update | SpMV | rhat.v | alpha | s update | SpMV | t.s, t.t | omega | x, r update | beta = 10, the
// same for every format and kernel mode (no SpMV kernel's fused dot is used).  Under a plan each of the two products with dinv
// becomes a cycle of C = precond_cycle_launches: 10 + 2 C under the sweeps; under the polynomial level 0's step 1 counts among C
// and rides in the two updates: 8 + 2 C (RightPrecond::apply_launches)
int sb_bicgstab_launches_per_body(const sb_bicgstab* s) { return 10 + 2 * s->pre.apply_launches(); }

template <int MODE> static void bicg_scalar_launch(sb_bicgstab* s)
{
  hipLaunchKernelGGL((bicg_scalar_k<MODE>), dim3(1), dim3(1024), 0, g.stream, s->nGroups, (const double*)s->l1a, (const double*)s->l1b, s->S,
      s->hist);
  HIP_CHECK(hipGetLastError());
}

// p and ph = M^-1 p (SECOND 0), s (in r's storage) and sh = M^-1 s (SECOND 1): the update with what rides in it, then what is
// left of the apply (a diagonal: nothing)
template <int SECOND> static void bicg_update_and_precond(sb_bicgstab* s)
{
  const uint32_t n = s->nr;
  if (!n) return;
  double* zh = SECOND ? s->sh : s->ph;
  if (SECOND) bicg_launch_update_s(n, s->r, s->v, s->r, s->pre.ride(), zh, s->S);
  else bicg_launch_update_p(n, s->r, s->p, s->v, s->pre.ride(), zh, s->S);
  HIP_CHECK(hipGetLastError());
  s->pre.apply(n, SECOND ? s->r : s->p, zh, &s->S->stop, true);
}

// one loop body
static void bicg_body(sb_bicgstab* s)
{
  const uint32_t n = s->nr;
  const int* stop  = &s->S->stop;
  const dim3 grid(vec_stream_grid(n)), block(1024);
  const BicgScalars* S = s->S;
  bicg_update_and_precond<0>(s);
  launch_spmv(s->A, s->ph, s->v, nullptr, stop);
  if (n) {
    hipLaunchKernelGGL(dot_l1_k, grid, block, 0, g.stream, n, (const double*)s->rhat, (const double*)s->v, s->l1a, stop);
    HIP_CHECK(hipGetLastError());
  }
  bicg_scalar_launch<1>(s);
  bicg_update_and_precond<1>(s);
  launch_spmv(s->A, s->sh, s->t, nullptr, stop);
  if (n) {
    hipLaunchKernelGGL(bicg_dot2_k, grid, block, 0, g.stream, n, (const double*)s->t, (const double*)s->r, s->l1a, s->l1b, stop);
    HIP_CHECK(hipGetLastError());
  }
  bicg_scalar_launch<2>(s);
  if (n) {
    hipLaunchKernelGGL(bicg_update_xr_k, grid, block, 0, g.stream, n, s->x, (const double*)s->ph, (const double*)s->sh, (const double*)s->r,
        (const double*)s->t, (const double*)s->rhat, s->r, S, s->l1a, s->l1b);
    HIP_CHECK(hipGetLastError());
  }
  bicg_scalar_launch<3>(s);
}

void sb_bicgstab_start(sb_bicgstab* s, int itermax, double eps)
{
  need_init();
  need_tree("sb_bicgstab_start", "BiCGStab", "sb_cg");
  s->pre.need_closed("sb_bicgstab_start");
  const int want = std::max(s->hist_cap, itermax + 2);
  grow(s->hist, s->hist_cap, want, 5);
  s->hist_cap   = want;
  BicgScalars h = zeroed<BicgScalars>(); // beta = omega = +0.0: the first body's p update is the general one
  h.itermax = itermax, h.eps = eps, h.hist_cap = s->hist_cap;
  write_block(s->S, &h);
  // prologue: x = 0, r = b, rhat = b, p = 0, v = 0, rho = rhat.r, rr = r.r, the loop test for k = 1
  const size_t nb = (size_t)s->nr * sizeof(double);
  HIP_CHECK(hipMemsetAsync(s->x, 0, nb, g.stream));
  HIP_CHECK(hipMemsetAsync(s->p, 0, nb, g.stream));
  HIP_CHECK(hipMemsetAsync(s->v, 0, nb, g.stream));
  if (s->nr) {
    HIP_CHECK(hipMemcpyAsync(s->r, s->b, nb, hipMemcpyDeviceToDevice, g.stream));
    HIP_CHECK(hipMemcpyAsync(s->rhat, s->b, nb, hipMemcpyDeviceToDevice, g.stream));
    hipLaunchKernelGGL(bicg_dot2_k, dim3(vec_stream_grid(s->nr)), dim3(1024), 0, g.stream, s->nr, (const double*)s->r, (const double*)s->rhat,
        s->l1a, s->l1b, (const int*)nullptr);
    HIP_CHECK(hipGetLastError());
  }
  bicg_scalar_launch<0>(s);
  s->k_next = 1;
  s->clock.begin();
}

void sb_bicgstab_run_iters(sb_bicgstab* s, int iters)
{
  need_init();
  s->clock.need_open("sb_bicgstab_run_iters", "sb_bicgstab_start");
  for (int i = 0; i < iters; i++) bicg_body(s), s->k_next++;
}

int sb_bicgstab_finish(sb_bicgstab* s)
{
  need_init();
  s->clock.need_open("sb_bicgstab_finish", "sb_bicgstab_start");
  s->clock.end();
  HIP_CHECK(hipStreamSynchronize(g.stream));
  s->clock.read();
  return read_block(s->S).iters + 1; // the value of k when the for loop exits
}

int sb_bicgstab_solve(sb_bicgstab* s, int itermax, double eps)
{
  sb_bicgstab_start(s, itermax, eps);
  sb_bicgstab_run_iters(s, loop_bodies(itermax));
  return sb_bicgstab_finish(s);
}

// which: 0 rr, 1 rho (both from the prologue on), 2 rv, 3 ts, 4 tt (one per body); returns the entries copied
int sb_bicgstab_history(const sb_bicgstab* s, int which, double* out, int cap)
{
  need_init();
  if (which < 0 || which > 4) SB_FATAL("sb_bicgstab_history: which = %d (0 rr, 1 rho, 2 rv, 3 ts, 4 tt)", which);
  const BicgScalars h = read_block(s->S);
  const int have      = which < 2 ? h.n_rr : which == 2 ? h.n_rv : h.n_ts;
  return copy_history(s->hist + (size_t)which * s->hist_cap, have, s->hist_cap, out, cap);
}

void sb_bicgstab_solution(const sb_bicgstab* s, double* x_host)
{
  need_init();
  download_original(s->A, s->x, x_host);
}
void sb_bicgstab_dinv(const sb_bicgstab* s, double* dinv_host)
{
  need_init();
  download_original(s->A, s->pre.diagonal(), dinv_host); // a plan's: level 0's, the borrowed handle's
}

// max|x - xexact| (solverCheckResidual, src/CGSolver.c:40-60); 0.0 without an exact solution
double sb_bicgstab_check_residual(const sb_bicgstab* s)
{
  need_init();
  return max_abs_diff_host(s->nr, s->x, s->xexact);
}

double sb_bicgstab_loop_ms(const sb_bicgstab* s) { return (double)s->clock.ms; }

// stop, iters, n_rr (= entries of rho too), n_rv, n_ts (= entries of tt too) of the device control block
void sb_bicgstab_counters(const sb_bicgstab* s, int out[5])
{
  const BicgScalars h = read_block(s->S);
  out[0] = h.stop, out[1] = h.iters, out[2] = h.n_rr, out[3] = h.n_rv, out[4] = h.n_ts;
}
