// sbhip_aggregation.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): the
// smoothed-aggregation prolongation made from the uploaded matrix alone (kernels: aggregation.hip.h).  Set-up work:
// nothing here runs inside a solver's loop.  The matrix is read in place, never downloaded; what crosses to the host is per-row
// counts and flags (the two prefix sums are the host's) and, at the end, the result.
// ===========================================================================
// aggregation and the smoothed prolongator
// ===========================================================================
namespace {
constexpr int AGG_BATCH = 4; // rounds enqueued between two reads of the undecided counters

struct AggRun {
  uint32_t n = 0, nAgg = 0, rounds = 0;
  uint64_t nStrong = 0;
  double *diag = nullptr, *dinv = nullptr; // device row order
  int32_t* agg = nullptr;                  // device, original numbering
  double ms[3] = { 0.0, 0.0, 0.0 };        // the graph's two launches, the rounds, the join passes
};
void agg_free(AggRun& R) { sb_free(R.diag), sb_free(R.dinv), sb_free(R.agg), R = AggRun(); }

struct AggTimer {
  hipEvent_t a, b;
  AggTimer()
  {
    HIP_CHECK(hipEventCreate(&a));
    HIP_CHECK(hipEventCreate(&b));
    HIP_CHECK(hipEventRecord(a, g.stream));
  }
  double stop()
  {
    float ms = 0.f;
    HIP_CHECK(hipEventRecord(b, g.stream));
    HIP_CHECK(hipEventSynchronize(b));
    HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    HIP_CHECK(hipEventDestroy(a));
    HIP_CHECK(hipEventDestroy(b));
    return (double)ms;
  }
};

// what both entries refuse before any launch
void agg_check_args(const char* fn, const sb_matrix* A, double theta)
{
  need_init();
  if (!A) SB_FATAL("%s: no matrix", fn);
  if (A->prec != 2) SB_FATAL("%s: double precision only (the matrix was uploaded in single precision)", fn);
  if (A->nr != A->nc)
    SB_FATAL("%s: the matrix is not square (%u rows, %u columns: halo columns of several ranks are not supported)", fn, A->nr, A->nc);
  if (!(theta >= 0.0 && theta < INFINITY)) SB_FATAL("%s: theta = %g: the strength threshold must be finite and not negative", fn, theta);
  // the diagonal and dinv, the neighbour list at its largest (every stored entry strong), three key buffers, the pointers, the
  // counts and the three aggregate buffers
  const double bytes = 16.0 * A->nr + 4.0 * (double)A->nnz + 24.0 * A->nr + 8.0 * ((double)A->nr + 1.0) + 12.0 * A->nr + 4096.0;
  const double have  = (double)sb_mem_free_bytes();
  if (bytes > have) SB_FATAL("%s: the aggregation needs %.0f bytes of device memory, %.0f are free", fn, bytes, have);
}

template <class X> void agg_graph_launch(bool fill, uint32_t n, const X& x, const AggMap& map, const double* diag, double theta2,
    uint32_t* count, const uint32_t* nbrPtr, uint32_t* nbr)
{
  const dim3 grid((n + 255) / 256), block(256);
  if (fill) hipLaunchKernelGGL((agg_graph_k<X, true>), grid, block, 0, g.stream, n, x, map, diag, theta2, count, nbrPtr, nbr);
  else hipLaunchKernelGGL((agg_graph_k<X, false>), grid, block, 0, g.stream, n, x, map, diag, theta2, count, nbrPtr, nbr);
  HIP_CHECK(hipGetLastError());
}
void agg_graph(bool fill, const sb_matrix* A, const double* diag, double theta2, uint32_t* count, const uint32_t* nbrPtr, uint32_t* nbr)
{
  const bool perm  = A->fmt == 1 && A->permuted;
  const AggMap map = { perm ? A->oldToNew : nullptr, perm ? A->newToOld : nullptr };
  if (A->fmt == 0) agg_graph_launch(fill, A->nr, GalCrs{ A->rowPtr, A->colInd, A->val }, map, diag, theta2, count, nbrPtr, nbr);
  else agg_graph_launch(fill, A->nr, GalSell{ A->chunkPtr, A->chunkLens, A->C, A->colInd, A->val }, map, diag, theta2, count, nbrPtr, nbr);
}

// the aggregates of A on the device; A has passed agg_check_args
AggRun agg_run(const char* fn, const sb_matrix* A, double theta)
{
  AggRun R;
  const uint32_t n = R.n = A->nr;
  if (n == 0) return R;
  const dim3 grid((n + 255) / 256), block(256);
  R.diag = (double*)sb_malloc((size_t)n * sizeof(double)), R.dinv = (double*)sb_malloc((size_t)n * sizeof(double));
  uint32_t bad[2] = { 0u, 0xFFFFFFFFu };
  uint32_t* dbad  = (uint32_t*)sb_malloc(sizeof bad);
  sb_h2d(dbad, bad, sizeof bad);
  launch_diagonal(A, R.diag, nullptr);
  hipLaunchKernelGGL(agg_dinv_k, grid, block, 0, g.stream, n, (const double*)R.diag, R.dinv, dbad);
  HIP_CHECK(hipGetLastError());
  sb_d2h(bad, dbad, sizeof bad);
  sb_free(dbad);
  if (bad[0])
    SB_FATAL("%s: %u of %u matrix rows have a diagonal entry that is zero or not finite (the first: device row %u): the strength "
             "test and the smoothing divide by it", fn, bad[0], n, bad[1]);

  // the strong graph: count, the host's prefix sum, fill
  const double theta2 = theta * theta;
  uint32_t* count     = (uint32_t*)sb_malloc((size_t)n * sizeof(uint32_t));
  AggTimer tg;
  agg_graph(false, A, R.diag, theta2, count, nullptr, nullptr);
  R.ms[0] = tg.stop();
  std::vector<uint32_t> cnt(n), ptr((size_t)n + 1, 0);
  sb_d2h(cnt.data(), count, (size_t)n * sizeof(uint32_t));
  sb_free(count);
  for (uint32_t i = 0; i < n; i++) R.nStrong += cnt[i], ptr[i + 1] = (uint32_t)R.nStrong;
  if (R.nStrong > (uint64_t)A->nnz) SB_FATAL("%s: %llu strong entries of %u stored ones", fn, (unsigned long long)R.nStrong, A->nnz);
  uint32_t* nbrPtr = sgs_to_device(ptr);
  uint32_t* nbr    = (uint32_t*)sb_malloc(((size_t)R.nStrong + 1) * sizeof(uint32_t));
  AggTimer tf;
  agg_graph(true, A, R.diag, theta2, nullptr, nbrPtr, nbr);
  R.ms[0] += tf.stop();

  // the rounds: every one reads `cur` and writes `nxt`; a batch's counters come back together
  uint64_t* key[2] = { (uint64_t*)sb_malloc((size_t)n * sizeof(uint64_t)), (uint64_t*)sb_malloc((size_t)n * sizeof(uint64_t)) };
  uint64_t* m1     = (uint64_t*)sb_malloc((size_t)n * sizeof(uint64_t));
  uint32_t* left   = (uint32_t*)sb_malloc(AGG_BATCH * sizeof(uint32_t));
  int cur          = 0;
  // every batch is timed alone, between its first and its last launch: the host's read-back of the counters is not in ms[1]
  AggTimer ti;
  hipLaunchKernelGGL(agg_init_k, grid, block, 0, g.stream, n, (const uint32_t*)nbrPtr, key[0]);
  HIP_CHECK(hipGetLastError());
  R.ms[1] = ti.stop();
  for (bool open = R.nStrong > 0; open;) {
    AggTimer tb;
    HIP_CHECK(hipMemsetAsync(left, 0, AGG_BATCH * sizeof(uint32_t), g.stream));
    for (int b = 0; b < AGG_BATCH; b++, cur ^= 1) {
      hipLaunchKernelGGL(agg_propagate_k, grid, block, 0, g.stream, n, (const uint32_t*)nbrPtr, (const uint32_t*)nbr,
          (const uint64_t*)key[cur], m1);
      hipLaunchKernelGGL(agg_decide_k, grid, block, 0, g.stream, n, (const uint32_t*)nbrPtr, (const uint32_t*)nbr,
          (const uint64_t*)key[cur], (const uint64_t*)m1, key[cur ^ 1], left + b);
    }
    HIP_CHECK(hipGetLastError());
    R.ms[1] += tb.stop();
    uint32_t h[AGG_BATCH];
    sb_d2h(h, left, sizeof h);
    for (int b = 0; b < AGG_BATCH && open; b++) {
      R.rounds++;
      if (h[b] == 0) open = false; // the rounds behind it in the batch changed nothing and do not count
    }
    if (R.rounds > n) SB_FATAL("%s: %u rounds over %u rows and rows are still undecided", fn, R.rounds, n);
  }

  // the roots in ascending row (the host's prefix sum), then both join passes
  uint32_t* root = (uint32_t*)sb_malloc((size_t)n * sizeof(uint32_t));
  hipLaunchKernelGGL(agg_roots_k, grid, block, 0, g.stream, n, (const uint64_t*)key[cur], root);
  HIP_CHECK(hipGetLastError());
  sb_d2h(cnt.data(), root, (size_t)n * sizeof(uint32_t));
  sb_free(root), sb_free(key[0]), sb_free(key[1]), sb_free(m1);
  std::vector<int32_t> num(n);
  for (uint32_t i = 0; i < n; i++) num[i] = cnt[i] ? (int32_t)R.nAgg++ : -1;
  int32_t* rootNum = sgs_to_device(num);
  int32_t* agg1    = (int32_t*)sb_malloc((size_t)n * sizeof(int32_t));
  R.agg            = (int32_t*)sb_malloc((size_t)n * sizeof(int32_t));
  AggTimer tj;
  HIP_CHECK(hipMemsetAsync(left, 0, sizeof(uint32_t), g.stream));
  hipLaunchKernelGGL(agg_join_k, grid, block, 0, g.stream, n, (const uint32_t*)nbrPtr, (const uint32_t*)nbr, (const int32_t*)rootNum, agg1);
  hipLaunchKernelGGL(agg_join_k, grid, block, 0, g.stream, n, (const uint32_t*)nbrPtr, (const uint32_t*)nbr, (const int32_t*)agg1, R.agg);
  hipLaunchKernelGGL(agg_check_k, grid, block, 0, g.stream, n, (const uint32_t*)nbrPtr, (const int32_t*)R.agg, left);
  HIP_CHECK(hipGetLastError());
  R.ms[2] = tj.stop();
  uint32_t stray = 0;
  sb_d2h(&stray, left, sizeof stray);
  sb_free(left), sb_free(rootNum), sb_free(agg1), sb_free(nbrPtr), sb_free(nbr);
  if (stray) SB_FATAL("%s: %u rows with strong entries found no aggregate within two hops", fn, stray);
  return R;
}
} // namespace

int sb_matrix_aggregate(const sb_matrix* A, double theta, int32_t* agg_out, uint32_t* n_agg, uint32_t* rounds)
{
  const char* fn = "sb_matrix_aggregate";
  agg_check_args(fn, A, theta);
  AggRun R = agg_run(fn, A, theta);
  if (agg_out && R.n) sb_d2h(agg_out, R.agg, (size_t)R.n * sizeof(int32_t));
  if (n_agg) *n_agg = R.nAgg;
  if (rounds) *rounds = R.rounds;
  agg_free(R);
  return 0;
}

sb_csr* sb_matrix_sa_prolongation(const sb_matrix* A, double theta, double omega_s, double lmax, uint32_t* n_agg)
{
  const char* fn = "sb_matrix_sa_prolongation";
  agg_check_args(fn, A, theta);
  if (!(omega_s >= 0.0 && omega_s < INFINITY)) SB_FATAL("%s: omega_s = %g: the smoothing weight must be finite and not negative", fn, omega_s);
  if (!(fabs(lmax) < INFINITY)) SB_FATAL("%s: lmax = %g is not finite", fn, lmax);
  AggRun R         = agg_run(fn, A, theta);
  const uint32_t n = R.n;
  if (R.nAgg == 0) SB_FATAL("%s: no root: every one of the %u rows is isolated (no strong entry at theta = %g), nothing to aggregate", fn, n, theta);
  // the tentative prolongator T: one entry of 1.0 per aggregated row
  std::vector<int32_t> agg(n);
  sb_d2h(agg.data(), R.agg, (size_t)n * sizeof(int32_t));
  sb_csr* c = new sb_csr();
  c->n      = n;
  c->ptr.assign((size_t)n + 1, 0);
  for (uint32_t i = 0; i < n; i++) {
    if (agg[i] >= 0) c->col.push_back((uint32_t)agg[i]);
    c->ptr[i + 1] = c->col.size();
  }
  c->val.assign(c->col.size(), 1.0);
  c->stats[0] = R.ms[0] + R.ms[1] + R.ms[2], c->stats[3] = (double)R.rounds, c->stats[4] = (double)R.nStrong;
  if (n_agg) *n_agg = R.nAgg;
  if (omega_s == 0.0) {
    c->stats[5] = 1.0;
    agg_free(R);
    return c;
  }
  if (!(lmax > 0.0)) lmax = poly_lmax_bound(poly_rowbound(A, R.dinv), fn, "");
  const double s = omega_s / lmax;
  // W = A T by the Galerkin product's stage 1, then the smoothing in place
  uint64_t* dTptr = sgs_to_device(c->ptr);
  uint32_t* dTcol = sgs_to_device(c->col);
  double* dTval   = sgs_to_device(c->val);
  GalOut W        = gal_stage1(fn, A, GalY{ dTptr, dTcol, dTval, n });
  sb_free(dTptr), sb_free(dTcol), sb_free(dTval);
  const bool perm = A->fmt == 1 && A->permuted;
  AggTimer ts;
  hipLaunchKernelGGL(agg_smooth_k, dim3((n + 255) / 256), dim3(256), 0, g.stream, n, (const uint64_t*)W.ptr, (const uint32_t*)W.col, W.val,
      (const int32_t*)R.agg, (const double*)R.dinv, (const uint32_t*)(perm ? A->oldToNew : nullptr), s);
  HIP_CHECK(hipGetLastError());
  c->stats[2] = ts.stop();
  c->col.resize(W.nnz), c->val.resize(W.nnz);
  sb_d2h(c->ptr.data(), W.ptr, c->ptr.size() * sizeof(uint64_t));
  if (W.nnz) sb_d2h(c->col.data(), W.col, (size_t)W.nnz * sizeof(uint32_t)), sb_d2h(c->val.data(), W.val, (size_t)W.nnz * sizeof(double));
  c->stats[1] = W.ms, c->stats[5] = (double)W.maxRow;
  gal_free(W);
  agg_free(R);
  return c;
}
