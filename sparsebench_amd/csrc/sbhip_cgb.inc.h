// sbhip_cgb.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): batched CG,
// nrhs independent CG solves on one pass over the matrix per body (kernels: batch.hip.h).  Double precision, one
// rank, tree dot order.  The batched path always streams the reference layout: the matrix's kernel mode (sb_matrix_use_packed)
// is ignored, the compressed mirror and the row programs are not used.
// ===========================================================================
// batched CG
// ===========================================================================
struct sb_cgb {
  const sb_matrix* A = nullptr;
  int nv = 0;
  uint32_t nr = 0, nc = 0, nGroups = 0;
  double *r = nullptr, *p = nullptr, *Ap = nullptr, *x = nullptr, *b = nullptr; // interleaved block vectors, device row order
  double* xexact = nullptr;  // column 0's exact solution, a plain vector in ORIGINAL row order (NULL: none)
  CgScalars* S = nullptr;    // one control block per column
  CgbControl* ctl = nullptr; // the global stop flag
  double *l1pAp = nullptr, *l1rr = nullptr; // nv * nGroups level-1 values each: column c at + c * nGroups
  double *rr_hist = nullptr, *pAp_hist = nullptr; // nv * hist_cap: column c at + c * hist_cap
  int hist_cap = 0;
  int k_next = 1;
  LoopClock clock;
};

#define CGB_WIDTHS "2, 4 or 8"
// CALL with NV a compile-time constant
#define CGB_DISPATCH(nv, CALL)                                                  \
  do {                                                                          \
    switch (nv) {                                                               \
    case 2: { constexpr int NV = 2; CALL; } break;                              \
    case 4: { constexpr int NV = 4; CALL; } break;                              \
    case 8: { constexpr int NV = 8; CALL; } break;                              \
    default: SB_FATAL("block width %d: the block kernels are built for " CGB_WIDTHS " right-hand sides", (int)(nv)); \
    }                                                                           \
  } while (0)

static void cgb_need_width(int nrhs, const char* fn)
{
  if (nrhs != 2 && nrhs != 4 && nrhs != 8)
    SB_FATAL("%s: nrhs = %d: the block kernels are built for " CGB_WIDTHS " right-hand sides (one right-hand side: sb_cg_create / sb_spmv_native)", fn, nrhs);
}
static bool spmmv_has_dot(const sb_matrix* m) { return m->fmt == 1 && m->C == 64; }

// rows in flight per lane of spmmv_scs64: chosen per width so that the kernel keeps NV accumulators and UNROLL * NV gathered
// values in registers without scratch (DESIGN 4.9 lists the resource figures)
template <int NV> struct SpmmvUnroll { static constexpr int value = NV == 8 ? 2 : 4; };

// Y = A X for a block vector; l1 != NULL (Sell-64 only): with the level-1 values of X_c . Y_c
static void launch_spmmv(const sb_matrix* m, int nv, const double* X, double* Y, double* l1, const int* stop)
{
  if (m->nr == 0) return;
  if (m->fmt == 1 && m->C == 64) {
    static int g_scs_nt = -1; // the batched kernel's own switch (SB_SCS_NT=0: plain loads; lab)
    if (g_scs_nt < 0) {
      const char* n = getenv("SB_SCS_NT");
      g_scs_nt      = n ? atoi(n) : 1;
    }
    const uint32_t nBlocks = (m->nChunks + 3) / 4;
    const uint32_t per     = scs_xcd() ? (nBlocks + 7) / 8 : 0;
    const dim3 grid(scs_xcd() ? per * 8 : nBlocks), block(256);
#define SPMMV_LAUNCH(D, N)                                                                                                       \
  hipLaunchKernelGGL((spmmv_scs64<NV, SpmmvUnroll<NV>::value, D, N>), grid, block, 0, g.stream, m->chunkPtr, m->chunkLens, m->colInd, \
      m->val, X, Y, m->nr, m->nChunks, per, l1, stop)
    CGB_DISPATCH(nv, {
      if (l1) { if (g_scs_nt) SPMMV_LAUNCH(true, true); else SPMMV_LAUNCH(true, false); }
      else { if (g_scs_nt) SPMMV_LAUNCH(false, true); else SPMMV_LAUNCH(false, false); }
    });
#undef SPMMV_LAUNCH
  } else {
    if (l1) SB_FATAL("the block kernel of this format has no fused dot");
    if (m->fmt == 0)
      CGB_DISPATCH(nv, hipLaunchKernelGGL(spmmv_crs_rows<NV>, dim3((m->nr + 255) / 256), dim3(256), 0, g.stream, m->rowPtr, m->colInd,
                           m->val, X, Y, m->nr, stop));
    else
      CGB_DISPATCH(nv, hipLaunchKernelGGL(spmmv_scs_rows<NV>, dim3((m->nrPadded + 255) / 256), dim3(256), 0, g.stream, m->chunkPtr,
                           m->chunkLens, m->colInd, m->val, X, Y, m->nr, m->nrPadded, m->C, stop));
  }
  HIP_CHECK(hipGetLastError());
}

// grid of block_vec_k over n rows: a wave per 256-row group, four waves per workgroup, 8 workgroups per CU at most
static uint32_t block_vec_grid(uint32_t n)
{
  const uint32_t nGroups = (n + 255u) >> 8;
  return std::max(1u, std::min((uint32_t)g.prop.multiProcessorCount * 8u, (nGroups + 3u) / 4u));
}
// grid of the two row kernels (cgb_update_p, cgb_x_finalize) over n rows: a thread per row, strip-mined past the cap
static uint32_t cgb_rows_grid(uint32_t n) { return stream_grid(n, 256); }

// OP of block_vec_k over n rows
static void launch_block_vec(int op, int nv, uint32_t n, const double* A, const double* B, double* R, const CgScalars* S, double* l1,
    const int* stop)
{
  if (n == 0) return;
  const dim3 grid(block_vec_grid(n)), block(256);
  CGB_DISPATCH(nv, {
    if (op == 0) hipLaunchKernelGGL((block_vec_k<NV, 0>), grid, block, 0, g.stream, n, A, B, R, S, l1, stop);
    else if (op == 1) hipLaunchKernelGGL((block_vec_k<NV, 1>), grid, block, 0, g.stream, n, A, B, R, S, l1, stop);
    else hipLaunchKernelGGL((block_vec_k<NV, 2>), grid, block, 0, g.stream, n, A, B, R, S, l1, stop);
  });
  HIP_CHECK(hipGetLastError());
}

// P_c = R_c + beta_c P_c (which != 0: R_c + 0.0 R_c) with the owed x update, over n rows
static void launch_cgb_update_p(int nv, uint32_t n, const double* R, double* P, double* X, const CgScalars* S, int which, const int* stop)
{
  if (n == 0) return;
  CGB_DISPATCH(nv, hipLaunchKernelGGL(cgb_update_p<NV>, dim3(cgb_rows_grid(n)), dim3(256), 0, g.stream, n, R, P, X, S, which, stop));
  HIP_CHECK(hipGetLastError());
}
// the x update every column's last body left owing, over n rows
static void launch_cgb_x_finalize(int nv, uint32_t n, double* X, const double* P, const CgScalars* S)
{
  if (n == 0) return;
  CGB_DISPATCH(nv, hipLaunchKernelGGL(cgb_x_finalize<NV>, dim3(cgb_rows_grid(n)), dim3(256), 0, g.stream, n, X, P, S));
  HIP_CHECK(hipGetLastError());
}

void sb_spmmv_native(const sb_matrix* m, int nrhs, const double* X_dev, double* Y_dev)
{
  need_init();
  SB_NEED_PREC(m, 2, "sb_spmmv_native");
  cgb_need_width(nrhs, "sb_spmmv_native");
  need_aligned16({ X_dev, Y_dev }, "sb_spmmv_native", "block vectors");
  launch_spmmv(m, nrhs, X_dev, Y_dev, nullptr, nullptr);
}

int sb_spmmv_native_dot(const sb_matrix* m, int nrhs, const double* X_dev, double* Y_dev, double* l1_dev)
{
  need_init();
  SB_NEED_PREC(m, 2, "sb_spmmv_native_dot");
  cgb_need_width(nrhs, "sb_spmmv_native_dot");
  need_aligned16({ X_dev, Y_dev }, "sb_spmmv_native_dot", "block vectors");
  if (!spmmv_has_dot(m)) return 0;
  launch_spmmv(m, nrhs, X_dev, Y_dev, l1_dev, nullptr);
  return 2;
}

void sb_block_interleave(const sb_matrix* m, int nrhs, const double* cols_dev, double* X_dev)
{
  need_init();
  SB_NEED_PREC(m, 2, "sb_block_interleave");
  cgb_need_width(nrhs, "sb_block_interleave");
  if (m->nr == 0) return;
  hipLaunchKernelGGL(block_interleave_k, dim3(stream_grid(m->nr, 256 / nrhs)), dim3(256), 0, g.stream, m->nr, nrhs,
      (const uint32_t*)(m->permuted ? m->newToOld : nullptr), cols_dev, X_dev);
  HIP_CHECK(hipGetLastError());
}
void sb_block_deinterleave(const sb_matrix* m, int nrhs, const double* X_dev, double* cols_dev)
{
  need_init();
  SB_NEED_PREC(m, 2, "sb_block_deinterleave");
  cgb_need_width(nrhs, "sb_block_deinterleave");
  if (m->nr == 0) return;
  hipLaunchKernelGGL(block_deinterleave_k, dim3(stream_grid(m->nr, 256 / nrhs)), dim3(256), 0, g.stream, m->nr, nrhs,
      (const uint32_t*)(m->permuted ? m->oldToNew : nullptr), X_dev, cols_dev);
  HIP_CHECK(hipGetLastError());
}

// algorithmic bytes of one SpMMV in the reference's layout: the matrix part of sb_matrix_spmv_bytes once, its vector part
// (y written, x read once) per right-hand side
double sb_matrix_spmmv_bytes(const sb_matrix* m, int nrhs)
{
  const double vec = m->fmt == 0 ? 8.0 * m->nr + 8.0 * m->nc : 8.0 * m->nrPadded + 8.0 * m->nc;
  return (sb_matrix_spmv_bytes(m) - vec) + (double)nrhs * vec;
}

sb_cgb* sb_cgb_create(const sb_matrix* m, sb_halo* halo, int nrhs, const double* B_host, const double* xexact0_host)
{
  need_init();
  cgb_need_width(nrhs, "sb_cgb_create");
  need_dp(m, "sb_cgb_create", "batched CG");
  need_one_rank(m, nullptr, "sb_cgb_create", "batched CG");
  need_tree("sb_cgb_create", "batched CG", "the single right-hand-side solver");
  (void)halo;
  sb_cgb* s = new sb_cgb();
  s->A = m, s->nv = nrhs, s->nr = m->nr, s->nc = m->nc;
  s->nGroups      = (m->nr + 255u) >> 8;
  const size_t vb = (size_t)m->nr * nrhs * sizeof(double), vbc = (size_t)m->nc * nrhs * sizeof(double);
  double** vecs[] = { &s->r, &s->Ap, &s->x, &s->b };
  for (double** v : vecs) *v = (double*)sb_malloc(vb + 4096);
  s->p = (double*)sb_malloc(vbc + 4096);
  // the caller's plain vectors, original row order, interleaved on the device: another layout than upload_permuted's
  double* tmp = scratch_ws(0, (size_t)m->nr * nrhs);
  if (m->nr) sb_h2d(tmp, B_host, vb);
  sb_block_interleave(m, nrhs, tmp, s->b);
  HIP_CHECK(hipStreamSynchronize(g.stream));
  if (xexact0_host) {
    s->xexact = (double*)sb_malloc((size_t)m->nr * sizeof(double) + 64);
    if (m->nr) sb_h2d(s->xexact, xexact0_host, (size_t)m->nr * sizeof(double));
  }
  s->S   = (CgScalars*)sb_malloc(sizeof(CgScalars) * nrhs);
  s->ctl = (CgbControl*)sb_malloc(sizeof(CgbControl));
  HIP_CHECK(hipMemsetAsync(s->S, 0, sizeof(CgScalars) * nrhs, g.stream));
  HIP_CHECK(hipMemsetAsync(s->ctl, 0, sizeof(CgbControl), g.stream));
  const size_t lb = ((size_t)nrhs * s->nGroups + 4) * sizeof(double);
  s->l1pAp = (double*)sb_malloc(lb), s->l1rr = (double*)sb_malloc(lb);
  HIP_CHECK(hipMemsetAsync(s->l1pAp, 0, lb, g.stream));
  HIP_CHECK(hipMemsetAsync(s->l1rr, 0, lb, g.stream));
  s->clock.create();
  return s;
}

void sb_cgb_free(sb_cgb* s)
{
  if (!s) return;
  HIP_CHECK(hipStreamSynchronize(g.stream));
  s->clock.destroy();
  sb_free(s->r), sb_free(s->p), sb_free(s->Ap), sb_free(s->x), sb_free(s->b), sb_free(s->xexact);
  sb_free(s->S), sb_free(s->ctl), sb_free(s->l1pAp), sb_free(s->l1rr), sb_free(s->rr_hist), sb_free(s->pAp_hist);
  delete s;
}

int sb_cgb_nrhs(const sb_cgb* s) { return s->nv; }

// launches per loop body: p update | SpMMV (+ p.Ap values) | alpha steps | r update (+ r.r values) | beta steps = 5 on Sell-64;
// a format whose block kernel has no fused dot adds the dot pass: 6
int sb_cgb_launches_per_body(const sb_cgb* s) { return spmmv_has_dot(s->A) ? 5 : 6; }

template <int MODE> static void cgb_scalar_launch(sb_cgb* s, const double* l1, int defer_x)
{
  hipLaunchKernelGGL((cgb_scalar_k<MODE>), dim3(s->nv), dim3(1024), 0, g.stream, s->nGroups, l1, s->S, s->ctl, s->rr_hist, s->pAp_hist,
      s->hist_cap, defer_x, s->nv);
  HIP_CHECK(hipGetLastError());
}

// Ap = A p with the level-1 values of p . Ap per column: in the SpMMV's epilogue, or the dot pass behind it
static void cgb_spmmv_and_pAp(sb_cgb* s, const int* stop)
{
  if (spmmv_has_dot(s->A)) {
    launch_spmmv(s->A, s->nv, s->p, s->Ap, s->l1pAp, stop);
  } else {
    launch_spmmv(s->A, s->nv, s->p, s->Ap, nullptr, stop);
    launch_block_vec(0, s->nv, s->nr, s->p, s->Ap, nullptr, nullptr, s->l1pAp, stop);
  }
}

// one loop body of solveCG (src/CGSolver.c:108-128) for every column, in the shape of the single solver's fused body
static void cgb_body(sb_cgb* s, int k)
{
  const int* stop = &s->ctl->stop;
  launch_cgb_update_p(s->nv, s->nr, s->r, s->p, s->x, s->S, k == 1 ? 1 : 0, stop);
  cgb_spmmv_and_pAp(s, stop);
  cgb_scalar_launch<2>(s, s->l1pAp, 0);
  launch_block_vec(1, s->nv, s->nr, s->Ap, nullptr, s->r, s->S, s->l1rr, stop);
  cgb_scalar_launch<1>(s, s->l1rr, 1);
}

void sb_cgb_start(sb_cgb* s, int itermax, double eps)
{
  need_init();
  need_tree("sb_cgb_start", "batched CG", "the single right-hand-side solver");
  const int nv = s->nv, want = std::max(s->hist_cap, itermax + 2);
  grow(s->rr_hist, s->hist_cap, want, nv);
  grow(s->pAp_hist, s->hist_cap, want, nv);
  s->hist_cap = want;
  std::vector<CgScalars> h(nv, zeroed<CgScalars>());
  for (CgScalars& c : h) c.itermax = itermax, c.eps = eps, c.hist_cap = s->hist_cap;
  write_block(s->S, h.data(), nv);
  HIP_CHECK(hipMemsetAsync(s->ctl, 0, sizeof(CgbControl), g.stream));
  // prologue, src/CGSolver.c:94-100: x0 = 0 (:28), p = 1.0 x + 0.0 x = 0, Ap = A p, r = 1.0 b + (-1.0) Ap, r.r, the loop test for k = 1
  HIP_CHECK(hipMemsetAsync(s->x, 0, (size_t)s->nr * nv * sizeof(double), g.stream));
  HIP_CHECK(hipMemsetAsync(s->p, 0, (size_t)s->nc * nv * sizeof(double), g.stream));
  launch_spmmv(s->A, nv, s->p, s->Ap, nullptr, nullptr);
  launch_block_vec(2, nv, s->nr, s->b, s->Ap, s->r, nullptr, s->l1rr, nullptr);
  cgb_scalar_launch<0>(s, s->l1rr, 0);
  s->k_next = 1;
  s->clock.begin();
}

void sb_cgb_run_iters(sb_cgb* s, int iters)
{
  need_init();
  s->clock.need_open("sb_cgb_run_iters", "sb_cgb_start");
  for (int i = 0; i < iters; i++) cgb_body(s, s->k_next++);
}

int sb_cgb_finish(sb_cgb* s)
{
  need_init();
  s->clock.need_open("sb_cgb_finish", "sb_cgb_start");
  s->clock.end();
  if (s->nr) { // the x update every column's last body left to "the next p update": nobody comes after it
    launch_cgb_x_finalize(s->nv, s->nr, s->x, s->p, s->S);
    hipLaunchKernelGGL(cgb_clear_pending, dim3(1), dim3(64), 0, g.stream, s->S, s->nv);
    HIP_CHECK(hipGetLastError());
  }
  HIP_CHECK(hipStreamSynchronize(g.stream));
  s->clock.read();
  int k = 0;
  for (int c = 0; c < s->nv; c++) k = std::max(k, sb_cgb_iterations(s, c));
  return k; // the largest k_c
}

int sb_cgb_solve(sb_cgb* s, int itermax, double eps)
{
  sb_cgb_start(s, itermax, eps);
  sb_cgb_run_iters(s, loop_bodies(itermax));
  return sb_cgb_finish(s);
}

static CgScalars cgb_column(const sb_cgb* s, int c, const char* fn)
{
  need_init();
  if (c < 0 || c >= s->nv) SB_FATAL("%s: column %d outside 0 .. %d", fn, c, s->nv - 1);
  return read_block(s->S + c);
}

// k_c: the value of k when column c's for loop exits (src/CGSolver.c:107,:140)
int sb_cgb_iterations(const sb_cgb* s, int c) { return cgb_column(s, c, "sb_cgb_iterations").iters + 1; }

int sb_cgb_history(const sb_cgb* s, int c, double* rr_out, int rr_cap, double* pAp_out, int pAp_cap, int* n_pAp)
{
  const CgScalars h = cgb_column(s, c, "sb_cgb_history");
  const int npa     = copy_history(s->pAp_hist + (size_t)c * s->hist_cap, h.n_pAp, s->hist_cap, pAp_out, pAp_cap);
  if (n_pAp) *n_pAp = npa;
  return copy_history(s->rr_hist + (size_t)c * s->hist_cap, h.n_rr, s->hist_cap, rr_out, rr_cap);
}

void sb_cgb_solution(const sb_cgb* s, int c, double* x_host)
{
  need_init();
  if (c < 0 || c >= s->nv) SB_FATAL("sb_cgb_solution: column %d outside 0 .. %d", c, s->nv - 1);
  if (s->nr == 0) return;
  double* tmp = scratch_ws(1, (size_t)s->nr * s->nv);
  sb_block_deinterleave(s->A, s->nv, s->x, tmp);
  sb_d2h(x_host, tmp + (size_t)c * s->nr, (size_t)s->nr * sizeof(double));
}

// max|x_c - xexact_c| (solverCheckResidual, src/CGSolver.c:40-60); only column 0 can have an exact solution: 0.0 otherwise
double sb_cgb_check_residual(const sb_cgb* s, int c)
{
  need_init();
  if (c < 0 || c >= s->nv) SB_FATAL("sb_cgb_check_residual: column %d outside 0 .. %d", c, s->nv - 1);
  if (c != 0 || !s->xexact || s->nr == 0) return 0.0;
  double* tmp = scratch_ws(1, (size_t)s->nr * s->nv);
  sb_block_deinterleave(s->A, s->nv, s->x, tmp); // column 0 leads the de-interleaved columns, in xexact's original row order
  return max_abs_diff_host(s->nr, tmp, s->xexact);
}

double sb_cgb_loop_ms(const sb_cgb* s) { return (double)s->clock.ms; }

// c >= 0: {stop, stop_next, iters, n_rr, n_pAp} of column c's control block; c = -1: {global stop, columns stopped, bodies
// enqueued since sb_cgb_start, 0, 0}
void sb_cgb_counters(const sb_cgb* s, int c, int out[5])
{
  if (c >= 0) {
    const CgScalars h = cgb_column(s, c, "sb_cgb_counters");
    out[0] = h.stop, out[1] = h.stop_next, out[2] = h.iters, out[3] = h.n_rr, out[4] = h.n_pAp;
    return;
  }
  const CgbControl h = read_block(s->ctl);
  out[0] = h.stop, out[1] = h.nStopped, out[2] = s->k_next - 1, out[3] = 0, out[4] = 0;
}

// --- blocking test entries: the vector kernels of the loop alone, launched by the loop's own launch functions ------------------
// grid of block_vec_k over n rows
void sb_block_vec_launch(uint32_t n, uint32_t out[3])
{
  need_init();
  out[0] = block_vec_grid(n), out[1] = 256u, out[2] = (uint32_t)g.prop.multiProcessorCount;
}
// grid of cgb_update_p and cgb_x_finalize over n rows
void sb_cgb_rows_launch(uint32_t n, uint32_t out[3])
{
  need_init();
  out[0] = cgb_rows_grid(n), out[1] = 256u, out[2] = (uint32_t)g.prop.multiProcessorCount;
}

// nrhs zeroed control blocks on the device, filled by `fill(block, column)`; freed by test_block_done
template <class F> static CgScalars* cgb_test_blocks(int nrhs, F fill)
{
  std::vector<CgScalars> h(nrhs, zeroed<CgScalars>());
  for (int c = 0; c < nrhs; c++) fill(h[c], c);
  CgScalars* S = (CgScalars*)sb_malloc(sizeof(CgScalars) * nrhs);
  write_block(S, h.data(), nrhs);
  return S;
}

void sb_block_vec_native(int op, int nrhs, uint32_t n, const double* A_dev, const double* B_dev, double* R_dev, const double* neg_alpha_host,
    const int* stop_host, double* l1_dev)
{
  need_init();
  cgb_need_width(nrhs, "sb_block_vec_native");
  if (op < 0 || op > 2) SB_FATAL("sb_block_vec_native: op = %d outside 0 .. 2", op);
  if (n == 0) return;
  need_aligned16({ A_dev, B_dev, R_dev }, "sb_block_vec_native", "block vectors");
  if (op != 1) { // as sb_cgb_start and the dot pass launch it: no control blocks
    launch_block_vec(op, nrhs, n, A_dev, B_dev, R_dev, nullptr, l1_dev, nullptr);
    HIP_CHECK(hipStreamSynchronize(g.stream));
    return;
  }
  CgScalars* S = cgb_test_blocks(nrhs, [&](CgScalars& h, int c) { h.neg_alpha = neg_alpha_host[c], h.stop = stop_host[c]; });
  CgbControl* ctl = test_block(zeroed<CgbControl>());
  launch_block_vec(1, nrhs, n, A_dev, nullptr, R_dev, S, l1_dev, &ctl->stop);
  test_block_done(S);
  sb_free(ctl);
}

void sb_cgb_update_p_native(int nrhs, uint32_t n, const double* R_dev, double* P_dev, double* X_dev, const double* beta_host,
    const double* alpha_host, const int* stop_host, const int* x_pending_host, int which)
{
  need_init();
  cgb_need_width(nrhs, "sb_cgb_update_p_native");
  if (n == 0) return;
  need_aligned16({ R_dev, P_dev, X_dev }, "sb_cgb_update_p_native", "block vectors");
  CgScalars* S = cgb_test_blocks(nrhs, [&](CgScalars& h, int c) {
    h.beta = beta_host[c], h.alpha = alpha_host[c], h.stop = stop_host[c], h.x_pending = x_pending_host[c];
  });
  CgbControl* ctl = test_block(zeroed<CgbControl>());
  launch_cgb_update_p(nrhs, n, R_dev, P_dev, X_dev, S, which, &ctl->stop);
  test_block_done(S);
  sb_free(ctl);
}

void sb_cgb_x_finalize_native(int nrhs, uint32_t n, double* X_dev, const double* P_dev, const double* alpha_host, const int* x_pending_host)
{
  need_init();
  cgb_need_width(nrhs, "sb_cgb_x_finalize_native");
  if (n == 0) return;
  need_aligned16({ X_dev, P_dev }, "sb_cgb_x_finalize_native", "block vectors");
  CgScalars* S = cgb_test_blocks(nrhs, [&](CgScalars& h, int c) { h.alpha = alpha_host[c], h.x_pending = x_pending_host[c]; });
  launch_cgb_x_finalize(nrhs, n, X_dev, P_dev, S);
  test_block_done(S);
}
