// sbhip_pcg.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): CG with a
// diagonal preconditioner (kernels: pcg.hip.h).  Double precision, tree dot order; one rank, or (the diagonal and the
// polynomial alone) several ranks over a halo plan.  The SpMV is the
// one the matrix's kernel mode selects (launch_spmv: the reference-layout stream or the masked row programs, with their
// fused p.Ap values; native CRS and generic C are followed by dot_l1_k).  The loop's vectors are allocations of the handle's
// own: the matrix's tuned arena (sb_matrix::vecArena) is laid out for sb_cg's vectors and stays with sb_cg.
// This file holds the handle and what does not ask how z is made; the loop, which does, is sbhip_pcg_loop.inc.h, included behind
// the preconditioners' files.
// ===========================================================================
// preconditioned CG
// ===========================================================================
struct sb_pcg {
  const sb_matrix* A = nullptr;
  uint32_t nr = 0, nc = 0, nGroups = 0;
  double *r = nullptr, *z = nullptr, *p = nullptr, *Ap = nullptr, *x = nullptr, *b = nullptr, *dinv = nullptr; // device row order
  double* xexact = nullptr;
  PcgScalars* S = nullptr;
  double *l1pAp = nullptr, *l1rz = nullptr, *l1rr = nullptr;
  double *rr_hist = nullptr, *rz_hist = nullptr, *pAp_hist = nullptr;
  int hist_cap = 0;
  int k_next = 1;
  LoopClock clock;
  // owned; NULL: the diagonal, which rides in pcg_update_r_k.  Else the sweeps, the polynomial or a V-cycle of either in its
  // place (sbhip_mg.inc.h); dinv is then 1 / diag(A) and level 0's
  struct PrecondPlan* pre = nullptr;
  // several ranks: the plan that fills the halo tail of every SpMV input, and the ranks' block (pcg.hip.h); NULL on
  // one rank
  sb_halo* halo  = nullptr;
  PcgRankSums* R = nullptr;
};
// the diagonal in the device's row order; bad_dev: NULL, or two uint32 (rows without a finite positive diagonal, the first of
// them) preset to {0, 0xFFFFFFFF}
static void launch_diagonal(const sb_matrix* m, double* d_dev, uint32_t* bad_dev)
{
  if (m->nr == 0) return;
  uint32_t* bad = bad_dev ? bad_dev : reinterpret_cast<uint32_t*>(scratch_partials(2));
  const dim3 grid((m->nr + 255) / 256), block(256);
  if (m->fmt == 0) hipLaunchKernelGGL(diag_crs_k, grid, block, 0, g.stream, m->nr, m->rowPtr, m->colInd, m->val, d_dev, bad);
  else
    hipLaunchKernelGGL(diag_scs_k, grid, block, 0, g.stream, m->nr, m->C, m->chunkPtr, m->chunkLens, m->colInd, m->val, d_dev, bad);
  HIP_CHECK(hipGetLastError());
}

void sb_matrix_diagonal(const sb_matrix* m, double* d_dev)
{
  need_init();
  SB_NEED_PREC(m, 2, "sb_matrix_diagonal");
  launch_diagonal(m, d_dev, nullptr);
}

// grid of pcg_update_r_k over n rows: vec_stream_grid
void sb_pcg_update_r_launch(uint32_t n, uint32_t out[3])
{
  need_init();
  out[0] = vec_stream_grid(n), out[1] = 1024u, out[2] = (uint32_t)g.prop.multiProcessorCount;
}

void sb_pcg_update_r_native(uint32_t n, double nalpha, const double* Ap_dev, double* r_dev, const double* dinv_dev, double* z_dev,
    double* l1_rz_dev, double* l1_rr_dev)
{
  need_init();
  if (n == 0) return;
  need_aligned16({ Ap_dev, r_dev, dinv_dev, z_dev }, "sb_pcg_update_r_native", "vectors");
  PcgScalars h  = zeroed<PcgScalars>();
  h.neg_alpha   = nalpha;
  PcgScalars* S = test_block(h);
  hipLaunchKernelGGL(pcg_update_r_k<0>, dim3(vec_stream_grid(n)), dim3(1024), 0, g.stream, n, Ap_dev, (const double*)r_dev, r_dev,
      dinv_dev, z_dev, (const PcgScalars*)S, l1_rz_dev, l1_rr_dev);
  test_block_done(S);
}

// The communicator's plane's local reduce (pcg_local_reduce_k) in one process: the level-1 values of a.b and, two != 0, of a.a
// over n rows by dot_l1_k, then the kernel; out: the block's two sums behind it, preset to { -1.0, -2.0 }: the kernel writes one
// (two == 0), both, or (stopped != 0: the block says the loop has exited) neither
void sb_pcg_local_reduce_native(uint32_t n, int two, int stopped, const double* a_dev, const double* b_dev, double out[2])
{
  need_init();
  need_aligned16({ a_dev, b_dev }, "sb_pcg_local_reduce_native", "vectors");
  const uint32_t m = (n + 255u) >> 8;
  double *la = (double*)sb_malloc(((size_t)m + 4) * sizeof(double)), *lb = (double*)sb_malloc(((size_t)m + 4) * sizeof(double));
  if (n) {
    hipLaunchKernelGGL(dot_l1_k, dim3(vec_stream_grid(n)), dim3(1024), 0, g.stream, n, a_dev, b_dev, la, (const int*)zero_flag());
    hipLaunchKernelGGL(dot_l1_k, dim3(vec_stream_grid(n)), dim3(1024), 0, g.stream, n, a_dev, a_dev, lb, (const int*)zero_flag());
  }
  PcgScalars h = zeroed<PcgScalars>();
  h.stop       = stopped ? 1 : 0;
  PcgScalars* S = test_block(h);
  PcgRankSums r = zeroed<PcgRankSums>();
  r.v[0] = -1.0, r.v[1] = -2.0;
  PcgRankSums* R = test_block(r);
  if (two) hipLaunchKernelGGL(pcg_local_reduce_k<true>, dim3(1), dim3(1024), 0, g.stream, m, (const double*)la, (const double*)lb, (const PcgScalars*)S, R);
  else hipLaunchKernelGGL(pcg_local_reduce_k<false>, dim3(1), dim3(1024), 0, g.stream, m, (const double*)la, (const double*)lb, (const PcgScalars*)S, R);
  r = read_block(R);
  out[0] = r.v[0], out[1] = r.v[1];
  test_block_done(S);
  sb_free(R), sb_free(la), sb_free(lb);
}

// precond: "Jacobi", or "SGS" / "MG (level l)", which have no caller's diagonal to fall back on
static bool dinv_host_allowed(const char* precond) { return precond[0] == 'J'; }
// dinv = 1 / diag(A) in the device's row order.  Rows without a finite positive diagonal are counted on the device, by
// diag_*_k's own predicate (BiCGStab's is another one, taken on the host: the two checks stay apart), and refused
static void jacobi_dinv(const sb_matrix* m, double* dinv_dev, const char* fn, const char* precond)
{
  if (!m->nr) return;
  double* tmp     = scratch_ws(0, m->nr);
  uint32_t bad[2] = { 0u, 0xFFFFFFFFu };
  uint32_t* dbad  = (uint32_t*)sb_malloc(sizeof bad);
  sb_h2d(dbad, bad, sizeof bad);
  launch_diagonal(m, tmp, dbad);
  sb_d2h(bad, dbad, sizeof bad);
  sb_free(dbad);
  if (bad[0])
    SB_FATAL("%s: %u of %u matrix rows have no finite positive diagonal entry (the first: device row %u): the %s "
             "preconditioner needs one in every row%s", fn, bad[0], m->nr, bad[1], precond,
        dinv_host_allowed(precond) ? "; pass dinv_host for another diagonal preconditioner" : "");
  hipLaunchKernelGGL(pcg_reciprocal_k, dim3(stream_grid(m->nr, 256)), dim3(256), 0, g.stream, m->nr, (const double*)tmp, dinv_dev);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(g.stream));
}

// Several ranks: the process is in a communicator of more than one rank and the caller gave the halo plan of this
// matrix.  Everything else is one rank's business, or need_one_rank's refusal
static bool pcg_several_ranks(const sb_matrix* m, const sb_halo* halo, const char* fn)
{
  if (!halo || !multi_rank() || sb_comm_size() < 2) return false;
  if (halo->nr != m->nr) SB_FATAL("%s: the halo plan has %u rows, the matrix %u", fn, halo->nr, m->nr);
  if (m->nr + (uint32_t)halo->externalCount != m->nc)
    SB_FATAL("%s: the halo plan receives %d entries, the matrix has %u halo columns", fn, halo->externalCount, m->nc - m->nr);
  return true;
}

// fn: the entry point as messages name it; precond: as jacobi_dinv takes it; ranksOk: the preconditioner runs on several ranks
static sb_pcg* pcg_create(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, const double* dinv_host,
    const char* fn, const char* precond, bool ranksOk)
{
  need_init();
  need_dp(m, fn, "PCG");
  const bool ranks = ranksOk && pcg_several_ranks(m, halo, fn);
  if (!ranks) need_one_rank(m, halo, fn, "PCG");
  need_tree(fn, "PCG", "sb_cg");
  if (dinv_host)
    for (uint32_t i = 0; i < m->nr; i++)
      if (!(dinv_host[i] > 0.0 && dinv_host[i] < INFINITY))
        SB_FATAL("%s: dinv[%u] = %g: the preconditioner's entries must be finite and positive", fn, i, dinv_host[i]);
  sb_pcg* s       = new sb_pcg();
  s->A = m, s->nr = m->nr, s->nc = m->nc;
  s->nGroups      = (m->nr + 255u) >> 8;
  const size_t nb = (size_t)m->nr * sizeof(double);
  double** vecs[] = { &s->r, &s->z, &s->Ap, &s->x, &s->b, &s->dinv, &s->p };
  for (double** v : vecs) *v = (double*)sb_malloc((size_t)m->nc * sizeof(double) + 4096);
  if (dinv_host) {
    upload_permuted(m, dinv_host, s->dinv);
  } else {
    jacobi_dinv(m, s->dinv, fn, precond);
  }
  upload_permuted(m, b_host, s->b);
  if (xexact_host) {
    s->xexact = (double*)sb_malloc(nb + 4096);
    upload_permuted(m, xexact_host, s->xexact);
  }
  s->S = (PcgScalars*)sb_malloc(sizeof(PcgScalars));
  HIP_CHECK(hipMemset(s->S, 0, sizeof(PcgScalars)));
  if (ranks) {
    s->halo = halo;
    s->R    = (PcgRankSums*)sb_malloc(sizeof(PcgRankSums));
    HIP_CHECK(hipMemset(s->R, 0, sizeof(PcgRankSums))); // never an uninitialised failure flag (sb_pcg_start points the push kernels at it)
  }
  // p.Ap: sized as sb_cg sizes the array its SpMV kernels write (4 per 256 rows, tail +0.0)
  const size_t lb = (4 * (size_t)s->nGroups + 4) * sizeof(double);
  double** l1s[]  = { &s->l1pAp, &s->l1rz, &s->l1rr };
  for (double** v : l1s) {
    *v = (double*)sb_malloc(lb);
    HIP_CHECK(hipMemsetAsync(*v, 0, lb, g.stream));
  }
  s->clock.create();
  HIP_CHECK(hipStreamSynchronize(g.stream));
  return s;
}

sb_pcg* sb_pcg_create(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, const double* dinv_host)
{
  return pcg_create(m, halo, b_host, xexact_host, dinv_host, "sb_pcg_create", "Jacobi", true);
}

int sb_pcg_history(const sb_pcg* s, double* rr_out, int rr_cap, double* rz_out, int rz_cap, double* pAp_out, int pAp_cap, int* n_pAp)
{
  need_init();
  const PcgScalars h = read_block(s->S);
  const int cap = std::min(rr_cap, rz_cap); // rr and rz come in pairs
  const int nrr = copy_history(s->rr_hist, h.n_rr, s->hist_cap, rr_out, cap);
  copy_history(s->rz_hist, h.n_rr, s->hist_cap, rz_out, cap);
  const int npa = copy_history(s->pAp_hist, h.n_pAp, s->hist_cap, pAp_out, pAp_cap);
  if (n_pAp) *n_pAp = npa;
  return nrr;
}

void sb_pcg_solution(const sb_pcg* s, double* x_host)
{
  need_init();
  download_original(s->A, s->x, x_host);
}
void sb_pcg_dinv(const sb_pcg* s, double* dinv_host)
{
  need_init();
  download_original(s->A, s->dinv, dinv_host);
}

// max|x - xexact| (solverCheckResidual, src/CGSolver.c:40-60), over every rank as sb_cg_check_residual takes it; 0.0 without an
// exact solution
double sb_pcg_check_residual(const sb_pcg* s)
{
  need_init();
  if (s->halo && (!s->xexact || s->nr == 0)) return 0.0; // (as sb_cg_check_residual: such a rank stays out of the reduction)
  double m = max_abs_diff_host(s->nr, s->x, s->xexact);
  if (s->halo) { // commReduction(&residual, MAX), src/CGSolver.c:55
    sb_h2d(g.scalar, &m, sizeof m);
    sb_comm_reduction(g.scalar, 0);
    sb_d2h(&m, g.scalar, sizeof m);
  }
  return m;
}

double sb_pcg_loop_ms(const sb_pcg* s) { return (double)s->clock.ms; }

// stop, stop_next, iters, n_rr (= entries of rz too), n_pAp of the device control block
void sb_pcg_counters(const sb_pcg* s, int out[5])
{
  const PcgScalars h = read_block(s->S);
  out[0] = h.stop, out[1] = h.stop_next, out[2] = h.iters, out[3] = h.n_rr, out[4] = h.n_pAp;
}
