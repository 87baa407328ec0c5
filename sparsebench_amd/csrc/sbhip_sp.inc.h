// sbhip_sp.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): single
// precision, the reference's FLOAT_TYPE=SP build (src/util.h:47-51).  Matrices, the reference-shaped operations and the CG loop
// on float data, over the kernels of kernels_sp.hip.h, on one rank or several (kernels_sp_comm.hip.h: float halo and float
// all-reduce on both data planes).  By default an SP matrix streams its reference layout.  With the switch below on
// (opt-in) an upload also builds the device-private mirror -- compressed tiles, masked row programs -- in float where EVERY
// chunk becomes a row program, and the loop multiplies through pack_sp.hip.h: spmv_prog_f32, and on one rank
// spmv_prog_fusep_f32 with the p update inside.  No placement tuner: its proxy is an fp64 loop body.
// ===========================================================================
// single precision
// ===========================================================================
// The process default of the SP mirror (include/sbhip.h: sb_sp_mirror): 0 off, 1 on.  SB_SP_MIRROR=0|1, read on first use --
// before sb_init too; anything else ends the process.  Consulted by the two uploads; a matrix keeps what it was built with.
static int g_spMirror = -1; // -1: not read yet
int sb_sp_mirror(void)
{
  if (g_spMirror < 0) {
    const char* e = getenv("SB_SP_MIRROR");
    if (!e || !*e || strcmp(e, "0") == 0) g_spMirror = 0;
    else if (strcmp(e, "1") == 0) g_spMirror = 1;
    else SB_FATAL("SB_SP_MIRROR=%s: expected 0 or 1", e);
  }
  return g_spMirror;
}
void sb_set_sp_mirror(int on)
{
  if (on != 0 && on != 1) SB_FATAL("sb_set_sp_mirror(%d): expected 0 (off) or 1 (on)", on);
  g_spMirror = on;
}

// the matrix-only part of spmv_fusep_possible: row programs for every chunk, no class dictionary, mapped or simple windows
static bool all_row_programs(const sb_matrix* pm)
{
  return pm && pm->mHdrs && pm->mDict == 0 && pm->nMaskedChunks == pm->nChunks && (pm->mSlotMap != nullptr || pm->mAllSimple);
}
int sb_matrix_all_row_programs(const sb_matrix* m) { return all_row_programs(m->fmt == 0 ? m->mirror : m) ? 1 : 0; }
static const char* why_not_all_row_programs(const sb_matrix* pm)
{
  if (!pm || !pm->mHdrs) return "no row programs (the pattern levels stop before level 6)";
  if (pm->mDict != 0 || pm->nMaskedChunks != pm->nChunks) return "chunks with per-lane code words";
  return "a window that is neither mapped nor simple";
}

// The builder of the mirror (sbhip_matrix.inc.h) never computes with matrix values, it only tells them apart -- by bit pattern:
// the dictionary, the pad test (__double_as_longlong(v) == 0), the pair keys and the program fit (build_masked's Ent::v is the
// 64-bit pattern) all work on the bits, and the host only copies the doubles.  So it runs unchanged on doubles whose element i
// holds float i's 32 bits ZERO-EXTENDED into the 64-bit pattern.  Not a numeric conversion: +0.0f becomes all-zero bits, the
// pad marker; -0.0f, subnormals, Inf and every NaN payload stay distinct and recoverable (a numeric widening would quiet
// signalling NaNs).  Every embedded double is +0.0 or a positive subnormal: should any host code compare them as numbers, that
// is bit equality as long as the host runs without denormals-are-zero -- the case for the Makefile's flags (-O3, no fast-math).
static std::vector<double> sp_embed(const float* v, size_t n)
{
  std::vector<double> d(n);
  for (size_t i = 0; i < n; i++) {
    uint32_t b;
    memcpy(&b, v + i, 4);
    const uint64_t w = b;
    memcpy(&d[i], &w, 8);
  }
  return d;
}

// ProgBlock -> ProgBlockF (pack_sp.hip.h: prog_narrow_k); the fp64 programs go
static void sp_narrow_programs(sb_matrix* pm)
{
  const uint32_t nb = pm->nProgBlocks;
  if (pm->mWindow > 256u * (pm->mCPT == 8 ? 15u : 12u) && pm->mSlotMap) SB_FATAL("mapped window of %u slots: more than a workgroup stages", pm->mWindow);
  HIP_CHECK(hipMalloc(&pm->mProgsF, (size_t)std::max(nb, 1u) * sizeof(ProgBlockF)));
  hipLaunchKernelGGL(prog_narrow_k, dim3((nb * 8u + 255u) / 256u + 1u), dim3(256), 0, g.stream, (const ProgBlock*)pm->mProgs, pm->mProgsF, nb);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(g.stream));
  sb_free(pm->mProgs);
  pm->mProgs = nullptr;
  pm->mBytes -= (double)(sizeof(ProgBlock) - sizeof(ProgBlockF)) * nb;
}

// everything the chain built on an SCS matrix goes; what scs_upload_common made stays: an upload with the switch off
static void sp_drop_mirror(sb_matrix* m)
{
  sb_free(m->pmeta), sb_free(m->pidx), sb_free(m->pcodes), sb_free(m->pdict);
  if (m->patSegs != m->tileSegs) sb_free(m->patSegs);
  sb_free(m->tileSegPtr), sb_free(m->tileSegs), sb_free(m->pslots);
  sb_free(m->rowBase), sb_free(m->tileClass), sb_free(m->jcodes), sb_free(m->classDict), sb_free(m->tileHdrs), sb_free(m->rowPats), sb_free(m->excRows);
  sb_free(m->mHdrs), sb_free(m->mStream), sb_free(m->mRowBase), sb_free(m->mProgs), sb_free(m->mProgsF), sb_free(m->mSlotMap);
  if (m->mOwnsTables) sb_free(m->mClassDict), sb_free(m->mSegs);
  sb_matrix b;
  b.prec = m->prec, b.fmt = m->fmt, b.nr = m->nr, b.nc = m->nc, b.nnz = m->nnz, b.C = m->C, b.sigma = m->sigma, b.nChunks = m->nChunks;
  b.nElems = m->nElems, b.nrPadded = m->nrPadded, b.permuted = m->permuted, b.chunkPtr = m->chunkPtr, b.chunkLens = m->chunkLens;
  b.colInd = m->colInd, b.valf = m->valf, b.oldToNew = m->oldToNew, b.newToOld = m->newToOld;
  *m = b;
}

static void sp_mirror_report(const sb_matrix* m, const char* reason)
{
  if (!(getenv("SB_SP_MIRROR_REPORT") && atoi(getenv("SB_SP_MIRROR_REPORT")) != 0)) return;
  const sb_matrix* pm = m->fmt == 0 ? m->mirror : m;
  const bool built    = pm && pm->mProgsF;
  fprintf(stderr, "SP_MIRROR built=%d fmt=%s chunks=%u programs=%u window=%u reason=%s\n", built ? 1 : 0, m->fmt == 0 ? "crs" : "scs",
      built ? pm->nChunks : (m->fmt == 1 ? m->nChunks : (m->nr + 63u) / 64u), built ? pm->nProgs : 0u, built ? pm->mWindow : 0u, reason);
}

sb_matrix* sb_crs_upload_f32(uint32_t nr, uint32_t nc, const uint32_t* rowPtr, const uint32_t* colInd, const float* val)
{
  need_init();
  need_float_allreduce("sb_crs_upload_f32");
  sb_matrix* m       = crs_upload_common(nr, nc, rowPtr, colInd, val, 1); // (no placement tuner: see the head of this file)
  const char* reason = "SB_SP_MIRROR / sb_set_sp_mirror is off";
  if (sb_sp_mirror()) { // the private Sell-64-1 mirror of build_crs_mirror, on the embedded values
    const std::vector<double> emb = sp_embed(val, m->nnz);
    build_crs_mirror(m, rowPtr, colInd, emb.data());
    if (all_row_programs(m->mirror)) {
      sp_narrow_programs(m->mirror);
      m->usePacked = 5; // (at every size)
      reason       = "every chunk is a row program";
    } else {
      reason = m->mirror ? why_not_all_row_programs(m->mirror) : "no pattern mirror (more than 255 distinct values, a stored +0.0 at column 0, or no row programs)";
      if (m->mirror) sb_matrix_free(m->mirror);
      m->mirror = nullptr, m->usePacked = 0;
    }
  }
  sp_mirror_report(m, reason);
  return m;
}

sb_matrix* sb_scs_upload_f32(uint32_t nr, uint32_t nc, uint32_t C, uint32_t sigma, uint32_t nChunks, uint32_t nElems,
    const uint32_t* chunkPtr, const uint32_t* chunkLens, const uint32_t* colInd, const float* val, const uint32_t* oldToNewPerm,
    const uint32_t* newToOldPerm)
{
  need_init();
  need_float_allreduce("sb_scs_upload_f32");
  sb_matrix* m = scs_upload_common(nr, nc, C, sigma, nChunks, nElems, chunkPtr, chunkLens, colInd, val, oldToNewPerm, newToOldPerm, 1);
  const char* reason = "SB_SP_MIRROR / sb_set_sp_mirror is off";
  if (sb_sp_mirror()) {
    if (C != 64) reason = "C != 64";
    else if (nChunks == 0 || nElems == 0 || nr == 0) reason = "empty matrix";
    else { // sb_scs_upload's chain, unchanged, on a temporary double copy of val that holds the floats' bit patterns
      const std::vector<double> emb = sp_embed(val, nElems);
      HIP_CHECK(hipMalloc(&m->val, ((size_t)nElems + SCS_SLACK) * sizeof(double)));
      HIP_CHECK(hipMemset(m->val + nElems, 0, SCS_SLACK * sizeof(double)));
      HIP_CHECK(hipMemcpy(m->val, emb.data(), (size_t)nElems * sizeof(double), hipMemcpyHostToDevice));
      build_packed(m, emb.data(), oldToNewPerm);
      build_lds_windows(m, chunkPtr, chunkLens, colInd, emb.data(), oldToNewPerm);
      build_patterns(m, chunkPtr, chunkLens, colInd, emb.data(), oldToNewPerm);
      product_modes_only(m);
      HIP_CHECK(hipStreamSynchronize(g.stream));
      sb_free(m->val);
      m->val = nullptr;
      if (all_row_programs(m)) {
        sp_narrow_programs(m);
        reason = "every chunk is a row program";
      } else { // kept only whole: no class tables, exception entries or per-lane code words in the float kernels
        reason = why_not_all_row_programs(m);
        sp_drop_mirror(m);
      }
    }
  }
  sp_mirror_report(m, reason);
  return m;
}

int sb_matrix_precision(const sb_matrix* m) { return m->prec; }

static float* sp_scratch(int which, size_t n) { return reinterpret_cast<float*>(scratch_ws(which, (n + 1) / 2)); }

// y = A x in the matrix's device row order; dotL1 != NULL (Sell-64 only): the level-1 values of x . y as well
// the float mirror is there and selected (mode 5): SCS the matrix itself, CRS its private Sell-64-1 mirror
static const sb_matrix* sp_mirror_selected(const sb_matrix* m)
{
  const sb_matrix* pm = m->fmt == 0 ? m->mirror : m;
  return m->usePacked == 5 && pm && pm->mProgsF ? pm : nullptr;
}
// pack_sp.hip.h: y = A x over the row programs (+ the level-1 values of x . y)
static void launch_prog_f32(const sb_matrix* pm, bool skipPad, const float* x, float* y, float* dotL1, const int* stop)
{
  const bool mapped = pm->mSlotMap != nullptr, dot = dotL1 != nullptr;
  const uint32_t count = pm->mNTiles, pper = (count + 7) / 8;
  const dim3 pgrid(pper * 8), block(256);
  const size_t shmem = (16 + (size_t)pm->mWindow) * sizeof(float);
  if (!stop) stop = zero_flag();
#define PF_LAUNCH(CP, DO, SK, MP)                                                                                         \
  SB_SPMV_LAUNCH((spmv_prog_f32<CP, DO, SK, MP>), pgrid, block, shmem, g.stream, pm->mHdrs, pm->mRowBase, pm->mProgsF,   \
      pm->mSlotMap, pm->mMapStride, x, y, pm->nr, pm->nChunks, count, pper, pm->padCol, dotL1, stop)
#define PF_PICK(CP, DO)                           \
  do {                                            \
    if (skipPad) {                                \
      if (mapped) PF_LAUNCH(CP, DO, true, true);  \
      else PF_LAUNCH(CP, DO, true, false);        \
    } else {                                      \
      if (mapped) PF_LAUNCH(CP, DO, false, true); \
      else PF_LAUNCH(CP, DO, false, false);       \
    }                                             \
  } while (0)
  if (pm->mCPT == 8) {
    if (dot) PF_PICK(8, true);
    else PF_PICK(8, false);
  } else {
    if (dot) PF_PICK(4, true);
    else PF_PICK(4, false);
  }
#undef PF_PICK
#undef PF_LAUNCH
  HIP_CHECK(hipGetLastError());
}
// pack_sp.hip.h: Ap = A p_new with p_new = r + beta p_old formed on the way (which != 0: the first body), x += alpha p_old
// where the previous body owes it, level-1 values of p_new . Ap into dotL1
static void launch_prog_fusep_f32(const sb_matrix* pm, bool skipPad, const float* pold, const float* r, float* pnew, float* xsol,
    float* y, const CgScalarsF* S, int which, float* dotL1)
{
  const bool mapped = pm->mSlotMap != nullptr;
  const uint32_t count = pm->mNTiles, pper = (count + 7) / 8;
  const dim3 pgrid(pper * 8), block(256);
  const size_t shmem = (16 + (size_t)pm->mWindow) * sizeof(float);
#define PFP_LAUNCH(CP, SK, MP)                                                                                                \
  SB_SPMV_LAUNCH((spmv_prog_fusep_f32<CP, SK, MP>), pgrid, block, shmem, g.stream, pm->mHdrs, pm->mRowBase, pm->mProgsF,      \
      pm->mSlotMap, pm->mMapStride, pold, r, pnew, xsol, y, S, which, pm->nr, pm->nChunks, count, pper, pm->padCol, dotL1)
#define PFP_PICK(CP)                          \
  do {                                        \
    if (skipPad) {                            \
      if (mapped) PFP_LAUNCH(CP, true, true); \
      else PFP_LAUNCH(CP, true, false);       \
    } else {                                  \
      if (mapped) PFP_LAUNCH(CP, false, true); \
      else PFP_LAUNCH(CP, false, false);      \
    }                                         \
  } while (0)
  if (pm->mCPT == 8) PFP_PICK(8);
  else PFP_PICK(4);
#undef PFP_PICK
#undef PFP_LAUNCH
  HIP_CHECK(hipGetLastError());
}

static void launch_spmv_f32(const sb_matrix* m, const float* x, float* y, float* dotL1, const int* stop)
{
  if (m->nr == 0) return;
  if (const sb_matrix* pm = sp_mirror_selected(m)) {
    launch_prog_f32(pm, m->fmt == 0, x, y, dotL1, stop);
    return;
  }
  if (m->fmt == 0) {
    if (dotL1) SB_FATAL("the single-precision CRS kernel has no fused dot: the CG loop adds a dot pass");
    if (m->tileRow) {
      const uint32_t per = (m->nCrsTiles + 7) / 8;
      SB_SPMV_LAUNCH(spmv_crs_split_f32, dim3(per * 8), dim3(CRS_THREADS), 0, g.stream, m->tileRow, m->rowPtr, m->colInd, m->valf,
          x, y, m->nCrsTiles, m->crsT, m->nnz, per, stop);
    } else {
      const uint32_t per = (m->nRowBlocks + 7) / 8;
      SB_SPMV_LAUNCH(spmv_crs_stream_f32, dim3(per * 8), dim3(CRS_THREADS), 0, g.stream, m->rowBlocks, m->rowPtr, m->colInd,
          m->valf, x, y, m->nRowBlocks, per, stop);
    }
  } else if (m->C == 64) {
    const uint32_t nBlocks = (m->nChunks + 3) / 4, per = (nBlocks + 7) / 8;
    if (dotL1)
      SB_SPMV_LAUNCH(spmv_scs64_f32<true>, dim3(per * 8), dim3(256), 0, g.stream, m->chunkPtr, m->chunkLens, m->colInd, m->valf, x,
          y, m->nr, m->nChunks, per, dotL1, stop);
    else
      SB_SPMV_LAUNCH(spmv_scs64_f32<false>, dim3(per * 8), dim3(256), 0, g.stream, m->chunkPtr, m->chunkLens, m->colInd, m->valf,
          x, y, m->nr, m->nChunks, per, (float*)nullptr, stop);
  } else {
    if (dotL1) SB_FATAL("fused dot is a Sell-64 feature");
    SB_SPMV_LAUNCH(spmv_scs_generic_f32, dim3((m->nrPadded + 255) / 256), dim3(256), 0, g.stream, m->chunkPtr, m->chunkLens,
        m->colInd, m->valf, x, y, m->nr, m->nrPadded, m->C, stop);
  }
  HIP_CHECK(hipGetLastError());
}

void sb_permute_f32(const sb_matrix* m, const float* in_orig, float* out_perm)
{
  need_init();
  SB_NEED_PREC(m, 1, "sb_permute_f32");
  if (!m->permuted) {
    if (in_orig != out_perm) sb_d2d(out_perm, in_orig, (size_t)m->nr * sizeof(float));
    return;
  }
  hipLaunchKernelGGL(gather_f32_k, dim3(stream_grid(m->nr, 256)), dim3(256), 0, g.stream, m->nr, m->newToOld, in_orig, out_perm);
  HIP_CHECK(hipGetLastError());
}

void sb_unpermute_f32(const sb_matrix* m, const float* in_perm, float* out_orig)
{
  need_init();
  SB_NEED_PREC(m, 1, "sb_unpermute_f32");
  if (!m->permuted) {
    if (in_perm != out_orig) sb_d2d(out_orig, in_perm, (size_t)m->nr * sizeof(float));
    return;
  }
  hipLaunchKernelGGL(gather_f32_k, dim3(stream_grid(m->nr, 256)), dim3(256), 0, g.stream, m->nr, m->oldToNew, in_perm, out_orig);
  HIP_CHECK(hipGetLastError());
}

void sb_spmv_f32(const sb_matrix* m, const float* x, float* y)
{
  need_init();
  SB_NEED_PREC(m, 1, "sb_spmv_f32");
  if (!m->permuted) {
    launch_spmv_f32(m, x, y, nullptr, nullptr);
    return;
  }
  float* xp = sp_scratch(0, m->nc);
  float* yp = sp_scratch(1, m->nr);
  sb_permute_f32(m, x, xp);
  if (m->nc > m->nr) sb_d2d(xp + m->nr, x + m->nr, (size_t)(m->nc - m->nr) * sizeof(float));
  launch_spmv_f32(m, xp, yp, nullptr, nullptr);
  sb_unpermute_f32(m, yp, y);
}

int sb_spmv_native_dot_f32(const sb_matrix* m, const float* x, float* y, float* l1_dev)
{
  need_init();
  SB_NEED_PREC(m, 1, "sb_spmv_native_dot_f32");
  if (!(m->fmt == 1 && m->C == 64) && !sp_mirror_selected(m)) {
    launch_spmv_f32(m, x, y, nullptr, nullptr);
    return 0;
  }
  launch_spmv_f32(m, x, y, l1_dev, nullptr);
  return 2;
}

// w = alpha x + beta y, waxpby's three branches (256-thread workgroups, stream_grid); stop != NULL: nothing on a set flag
static void launch_sp_waxpby(uint32_t n, float alpha, const float* x, float beta, const float* y, float* w, const int* stop)
{
  if (n == 0) return;
  hipLaunchKernelGGL(waxpby_f32_k, dim3(stream_grid(n, 256)), dim3(256), 0, g.stream, n, alpha, x, beta, y, w, stop);
  HIP_CHECK(hipGetLastError());
}

void sb_waxpby_f32(uint32_t n, float alpha, const float* x, float beta, const float* y, float* w)
{
  need_init();
  launch_sp_waxpby(n, alpha, x, beta, y, w, nullptr);
}

static void launch_dot_l0_f32(uint32_t n, const float* a, const float* b, float* partials, const int* stop)
{
  if (n == 0) return;
  const uint32_t nG = ((n + 255u) >> 8) * 4u;
  hipLaunchKernelGGL(dot_l0_f32_k, dim3(stream_grid(nG, 4)), dim3(256), 0, g.stream, n, a, b, partials, stop);
  HIP_CHECK(hipGetLastError());
}
static void launch_dot_seq_f32(uint32_t n, const float* a, const float* b, const uint32_t* perm, float* out, const int* stop)
{
  hipLaunchKernelGGL(dot_seq_f32_k, dim3(1), dim3(1024), 0, g.stream, n, a, b, perm, out, stop);
  HIP_CHECK(hipGetLastError());
}

void sb_ddot_partials_f32(uint32_t n, const float* x, const float* y, float* partials_dev)
{
  need_init();
  launch_dot_l0_f32(n, x, y, partials_dev, nullptr);
}

void sb_reduce_final_f32(uint32_t m, const float* partials_dev, float* result_dev)
{
  need_init();
  hipLaunchKernelGGL(reduce_final_f32_k, dim3(1), dim3(1024), 0, g.stream, m, partials_dev, result_dev, 0);
  HIP_CHECK(hipGetLastError());
}

float sb_ddot_f32(uint32_t n, const float* x, const float* y)
{
  need_init();
  float* res = reinterpret_cast<float*>(g.scalar);
  if (sb_dot_order() == 1) {
    launch_dot_seq_f32(n, x, y, nullptr, res, nullptr);
  } else {
    const uint32_t m = (n + 255u) / 256u;
    float* q         = reinterpret_cast<float*>(scratch_partials(2 * (size_t)m + 1));
    sb_ddot_partials_f32(n, x, y, q);
    sb_reduce_final_f32(m, q, res);
  }
  if (multi_rank()) sb_comm_reduction_f32(res, 1); // commReduction(&sum, SUM), src/solver.c:60
  float r = 0.f;
  sb_d2h(&r, res, sizeof r);
  return r;
}

// ---- CG in single precision (src/CGSolver.c:62-141 of the SP build) ------------------------------------------------------------
// The same loop shapes as fp64, in float:
//   fused (tree order, the default): p update with the beta step at its head and the owed x update | SpMV with the p.Ap level-1
//     values (Sell-64; CRS and generic C: SpMV, then a level-1 dot pass) | r update with the alpha step and the r.r level-1
//     values -- 3 launches per body on Sell-64, 4 otherwise;
//   the reference's op list (fused = 0, and always under seq): waxpby, spMVM and ddot as separate launches, every dot either the
//     tree order's level-0 partials or the sequential sum.
// Both give the same bits under the tree order.
// Several ranks (src/CGSolver.c:122 commExchange, src/solver.c:60 commReduction): the halo exchange of p in front of the SpMV,
// and every dot all-reduced before its scalar step -- so the steps cannot ride in their consumers (there is no
// cg_update_p_f32<1> / cg_update_r_f32<1> here): the fused body is
//   peer-mapped plane:    p update | push | pull | SpMV (+ p.Ap level 1) | alpha (cg_scalar_p2p_f32_k) | r update (+ r.r
//                         level 1) | beta (cg_scalar_p2p_f32_k) -- 7 launches on Sell-64, 8 with the dot pass of CRS / generic C;
//   communicator's plane: halo pack (+ the unpack of a host transport) in front of the send / recv, and each dot as local
//                         reduce (cg_local_f32_k) | all-reduce (sb_comm_reduction_f32) | apply (cg_apply_local_f32_k).
// SP has no SpMV that forms p itself on several ranks (no spmv_prog_fusep there), so sb_comm_halo_push_inside has nothing to ride
// on here.  With sb_comm_halo_fold(1) the Sell-64 body on the peer-mapped plane is cg_update_p_push_f32 | spmv_scs64_halo_f32 |
// alpha | r update | beta -- 5 launches: the push in the p update, the pull in the SpMV's halo blocks (sbhip_cg.inc.h:
// halo_fold_plan; kernels_sp_comm.hip.h).
sb_cg* sb_cg_create_f32(const sb_matrix* m, sb_halo* halo, const float* b_host, const float* xexact_host)
{
  need_init();
  SB_NEED_PREC(m, 1, "sb_cg_create_f32");
  need_float_allreduce("sb_cg_create_f32");
  sb_cg* s = new sb_cg();
  s->prec = 1, s->A = m, s->halo = halo, s->nr = m->nr, s->nc = m->nc;
  if (halo && halo->nr != m->nr) SB_FATAL("halo plan and matrix disagree on nr");
  if (halo && m->nr + (uint32_t)halo->externalCount != m->nc) SB_FATAL("halo externalCount != nc-nr");
  const size_t nb = (size_t)m->nr * sizeof(float);
  s->rf = (float*)sb_malloc(nb), s->Apf = (float*)sb_malloc(nb), s->xf = (float*)sb_malloc(nb), s->bf = (float*)sb_malloc(nb);
  s->pf = (float*)sb_malloc((size_t)m->nc * sizeof(float));
  float* tmp = sp_scratch(0, m->nr);
  sb_h2d(tmp, b_host, nb);
  sb_permute_f32(m, tmp, s->bf);
  if (xexact_host) {
    s->xexactf = (float*)sb_malloc(nb);
    HIP_CHECK(hipStreamSynchronize(g.stream));
    sb_h2d(tmp, xexact_host, nb);
    sb_permute_f32(m, tmp, s->xexactf);
  }
  HIP_CHECK(hipStreamSynchronize(g.stream));
  s->SF = (CgScalarsF*)sb_malloc(sizeof(CgScalarsF));
  HIP_CHECK(hipMemset(s->SF, 0, sizeof(CgScalarsF)));
  s->XF = (CgCommF*)sb_malloc(sizeof(CgCommF));
  HIP_CHECK(hipMemset(s->XF, 0, sizeof(CgCommF)));
  s->nPartials  = (m->nr + 255) / 256;
  const size_t np = (4 * (size_t)s->nPartials + 4) * sizeof(float);
  s->partialsF = (float*)sb_malloc(np), s->partials2F = (float*)sb_malloc(np);
  HIP_CHECK(hipMemset(s->partialsF, 0, np));
  HIP_CHECK(hipMemset(s->partials2F, 0, np));
  s->fused = 1, s->timing = false, s->evUsed = 0, s->loop_ms = 0.f, s->spmvTiming = false, s->spmvEvUsed = 0;
  s->k_next = 1, s->started = false, s->hist_cap = 0;
  HIP_CHECK(hipEventCreate(&s->evLoop0));
  HIP_CHECK(hipEventCreate(&s->evLoop1));
  for (double& v : s->region_ms) v = 0.0;
  apply_dot_order(s);
  return s;
}

static void sp_cg_free_arrays(sb_cg* s)
{
  halo_push_watch(s->halo, &s->XF->p2p_error, false);
  sb_free(s->XF);
  sb_free(s->rf), sb_free(s->pf), sb_free(s->pf2), sb_free(s->Apf), sb_free(s->xf), sb_free(s->bf), sb_free(s->xexactf);
  sb_free(s->SF), sb_free(s->partialsF), sb_free(s->partials2F), sb_free(s->rrHistF), sb_free(s->pApHistF);
}

static bool sp_spmv_has_dot(const sb_cg* s) { return (s->A->fmt == 1 && s->A->C == 64) || sp_mirror_selected(s->A); }
// The p update inside the SpMV (pack_sp.hip.h: spmv_prog_fusep_f32; body = SpMV | r update with the alpha step | beta step): one
// rank, the fused tree-order loop, the float mirror selected, and the wish (sb_cg_set_fuse_p, SB_FUSE_P, else the library's
// default).  Inside a solve the answer is the one sp_cg_start latched, as fusep_plan does for fp64: the fused path keeps p
// double-buffered, the in-place path does not, and the pieces of one solve must not mix them.
static bool sp_fusep_plan(sb_cg* s)
{
  if (s->started && s->fusepLatched >= 0) return s->fusepLatched > 0;
  if (s->fusepPlan < 0) {
    const char* env = getenv("SB_FUSE_P");
    s->fusepPlan    = (s->fusepWant >= 0 ? s->fusepWant != 0 : env ? atoi(env) != 0 : SB_FUSE_P_DEFAULT) ? 1 : 0;
  }
  // (nc == nr: the kernel forms p_new for every window column from r, which has nr entries)
  return s->fusepPlan > 0 && s->fused == 1 && s->nr > 0 && s->nc == s->nr && !multi_rank() && sp_mirror_selected(s->A) != nullptr;
}
static int sp_launches_per_body(const sb_cg* s)
{
  if (!s->fused) return 0;
  if (!multi_rank()) return sp_fusep_plan(const_cast<sb_cg*>(s)) || sp_spmv_has_dot(s) ? 3 : 4;
  int n = sp_spmv_has_dot(s) ? 5 : 6; // p update | SpMV | (dot pass) | alpha | r update | beta
  if (const sb_halo* h = s->halo) {
    if (halo_p2p_active(h)) n += (h->totalSend ? 1 : 0) + (h->indegree ? 1 : 0); // push, pull
    else n += (h->totalSend ? 1 : 0) + (g.hasXport && h->externalCount ? 1 : 0); // pack (+ the host transport's unpack)
  }
  if (!p2p_dots()) n += 2; // local reduce | all-reduce | apply: one launch more per dot
  return n;
}

// ---- the launches of the loop's vector and scalar kernels, on plain pointers: the loop below and the blocking test entries at
// the end of this file both go through them, so a test of an entry is a test of the loop's launch ----------------
// cg_update_p_f32 / cg_update_p_push_f32: four floats per thread, 1024 threads, at most two workgroups per CU
static uint32_t sp_update_p_grid(uint32_t n)
{
  const uint32_t vb = 1024u, capV = (uint32_t)g.prop.multiProcessorCount * 2u;
  return std::max(1u, std::min(capV, (n / 4 + vb) / vb));
}
// a wave per aligned 256 rows, 16 waves per workgroup, at most wgPerCu workgroups per CU (cg_update_r_f32: 1, dot_l1_f32_k: 2)
static uint32_t sp_groups_grid(uint32_t n, uint32_t wgPerCu)
{
  const uint32_t nG = (n + 255u) >> 8;
  return std::max(1u, std::min((uint32_t)g.prop.multiProcessorCount * wgPerCu, (nG + 15u) / 16u));
}
// cg_update_p_f32<mode>: mode 0 p = r + beta p (which != 0: r + 0.0 r) with the owed x update; mode 1 with the beta step at its
// head, from the m level-1 values l1 -- launched at n = 0 too: the step is the loop's
static void launch_sp_update_p(int mode, uint32_t n, const float* r, float* p, float* x, CgScalarsF* S, int which, uint32_t m,
    const float* l1, float* rr_hist)
{
  const dim3 grid(sp_update_p_grid(n)), block(1024);
  if (mode == 1) hipLaunchKernelGGL(cg_update_p_f32<1>, grid, block, 0, g.stream, n, r, p, x, S, which, m, l1, rr_hist);
  else if (n) hipLaunchKernelGGL(cg_update_p_f32<0>, grid, block, 0, g.stream, n, r, p, x, S, which, 0u, (const float*)nullptr, (float*)nullptr);
  HIP_CHECK(hipGetLastError());
}
// cg_update_r_f32<mode>: mode 0 r += neg_alpha Ap unless *stop; mode 1 with the alpha step at its head, from the m level-1 values
// l1in; the level-1 values of r.r into l1out
static void launch_sp_update_r(int mode, uint32_t n, const float* Ap, float* r, CgScalarsF* S, float* l1out, const int* stop, uint32_t m,
    const float* l1in, float* rr_hist, float* pAp_hist)
{
  const dim3 grid(sp_groups_grid(n, 1)), block(1024);
  if (mode == 1) hipLaunchKernelGGL(cg_update_r_f32<1>, grid, block, 0, g.stream, n, Ap, r, S, l1out, stop, m, l1in, rr_hist, pAp_hist);
  else
    hipLaunchKernelGGL(cg_update_r_f32<0>, grid, block, 0, g.stream, n, Ap, r, S, l1out, stop, 0u, (const float*)nullptr, (float*)nullptr,
        (float*)nullptr);
  HIP_CHECK(hipGetLastError());
}
// the level-1 values of a . b, one per aligned 256 elements
static void launch_sp_dot_l1(uint32_t n, const float* a, const float* b, float* l1out, const int* stop)
{
  if (n == 0) return;
  hipLaunchKernelGGL(dot_l1_f32_k, dim3(sp_groups_grid(n, 2)), dim3(1024), 0, g.stream, n, a, b, l1out, stop);
  HIP_CHECK(hipGetLastError());
}
// w = x + (*a_dev) y of the reference-shaped op list
static void launch_sp_axpy_sdev(uint32_t n, const float* x, const float* a_dev, const float* y, float* w, const int* stop)
{
  if (n == 0) return;
  hipLaunchKernelGGL(axpy_sdev_f32_k, dim3(stream_grid(n, 256)), dim3(256), 0, g.stream, n, x, a_dev, y, w, stop);
  HIP_CHECK(hipGetLastError());
}
// the x update the last body left owing; p1 != NULL: p double-buffered, p0 / p1 the buffers of the even / odd bodies
static void launch_sp_x_finalize(uint32_t n, float* x, const float* p0, const float* p1, const CgScalarsF* S)
{
  if (n == 0) return;
  if (p1) hipLaunchKernelGGL(cg_x_finalize2_f32, dim3(stream_grid(n, 256)), dim3(256), 0, g.stream, n, x, p0, p1, S);
  else hipLaunchKernelGGL(cg_x_finalize_f32, dim3(stream_grid(n, 256)), dim3(256), 0, g.stream, n, x, p0, S);
  HIP_CHECK(hipGetLastError());
}
// the scalar step `mode` on one rank: levels 1-2 of the dot in q + the step, one workgroup
static void launch_sp_scalar(int mode, uint32_t m, const float* q, CgScalarsF* S, float* rr_hist, float* pAp_hist, int defer_x, int l1)
{
  const dim3 grid(1), block(1024);
  if (mode == 0) hipLaunchKernelGGL((cg_scalar_f32_k<0>), grid, block, 0, g.stream, m, q, S, rr_hist, pAp_hist, defer_x, l1);
  else if (mode == 1) hipLaunchKernelGGL((cg_scalar_f32_k<1>), grid, block, 0, g.stream, m, q, S, rr_hist, pAp_hist, defer_x, l1);
  else if (mode == 2) hipLaunchKernelGGL((cg_scalar_f32_k<2>), grid, block, 0, g.stream, m, q, S, rr_hist, pAp_hist, defer_x, l1);
  else SB_FATAL("launch_sp_scalar: unknown mode %d", mode);
  HIP_CHECK(hipGetLastError());
}
// ... and split for the communicator's plane: levels 1-2 into X->local | (the all-reduce) | the step on X->local
static void launch_sp_local(uint32_t m, const float* q, const CgScalarsF* S, CgCommF* X, int l1)
{
  hipLaunchKernelGGL(cg_local_f32_k, dim3(1), dim3(1024), 0, g.stream, m, q, S, X, l1);
  HIP_CHECK(hipGetLastError());
}
static void launch_sp_apply_local(int mode, CgScalarsF* S, const CgCommF* X, float* rr_hist, float* pAp_hist, int defer_x)
{
  const dim3 grid(1), block(64);
  if (mode == 0) hipLaunchKernelGGL((cg_apply_local_f32_k<0>), grid, block, 0, g.stream, S, X, rr_hist, pAp_hist, defer_x);
  else if (mode == 1) hipLaunchKernelGGL((cg_apply_local_f32_k<1>), grid, block, 0, g.stream, S, X, rr_hist, pAp_hist, defer_x);
  else if (mode == 2) hipLaunchKernelGGL((cg_apply_local_f32_k<2>), grid, block, 0, g.stream, S, X, rr_hist, pAp_hist, defer_x);
  else SB_FATAL("launch_sp_apply_local: unknown mode %d", mode);
  HIP_CHECK(hipGetLastError());
}

// one dot of the reference's op list into partialsF: tree level-0 partials, or (seq) the sequential sum in original row order
static void sp_dot(sb_cg* s, const float* a, const float* b, const int* stop)
{
  if (s->seqLatched > 0) launch_dot_seq_f32(s->nr, a, b, s->A->permuted ? s->A->oldToNew : nullptr, s->partialsF, stop);
  else launch_dot_l0_f32(s->nr, a, b, s->partialsF, stop);
}
// levels 1-2 of the dot in q + the scalar step (seq: q[0] is the whole sum); several ranks: with the all-reduce of the rank sums
// in between -- inside the step's launch (peer-mapped), or local reduce | sb_comm_reduction_f32 | apply (the communicator's)
template <int MODE> static void sp_scalar(sb_cg* s, const float* q, int l1, int defer_x)
{
  uint32_t m = s->nPartials;
  if (s->seqLatched > 0) m = 1, l1 = 1;
  if (!multi_rank()) {
    launch_sp_scalar(MODE, m, q, s->SF, s->rrHistF, s->pApHistF, defer_x, l1);
    return;
  }
  if (p2p_dots()) {
    hipLaunchKernelGGL((cg_scalar_p2p_f32_k<MODE>), dim3(1), dim3(1024), 0, g.stream, m, q, s->SF, s->XF, s->rrHistF, s->pApHistF,
        defer_x, (const P2PView*)g.p2pView, ++g.p2pSeq, l1, (const int*)(s->halo && s->halo->p2p ? s->halo->err : nullptr));
    HIP_CHECK(hipGetLastError());
    return;
  }
  launch_sp_local(m, q, s->SF, s->XF, l1);
  mark(s, R_DDOT);
  sb_comm_reduction_f32(&s->XF->local, 1);
  mark(s, R_COMM);
  launch_sp_apply_local(MODE, s->SF, s->XF, s->rrHistF, s->pApHistF, defer_x);
}
static void sp_flush_beta(sb_cg* s)
{
  if (!s->betaFold) return;
  sp_scalar<1>(s, s->partials2F, 1, 1);
  mark(s, R_DDOT);
  phase_mark(s, PH_BETA);
  s->betaFold = 0;
}

// several ranks: the all-reduced alpha step | r update (+ the level-1 values of r.r) | the all-reduced beta step / loop test
// (x += alpha p stays owed)
static void sp_alpha_r_beta(sb_cg* s)
{
  sp_scalar<2>(s, s->partialsF, 1, 0);
  mark(s, R_DDOT);
  phase_mark(s, PH_ALPHA);
  launch_sp_update_r(0, s->nr, s->Apf, s->rf, s->SF, s->partials2F, &s->SF->stop, 0u, nullptr, nullptr, nullptr);
  mark(s, R_WAXPBY);
  phase_mark(s, PH_R_UPDATE);
  sp_scalar<1>(s, s->partials2F, 1, 1);
  mark(s, R_DDOT);
  phase_mark(s, PH_BETA);
}

static void sp_loop_body(sb_cg* s, int k)
{
  const uint32_t n = s->nr;
  const int* stop  = &s->SF->stop;
  if (sp_fusep_plan(s)) {
    // p = r + beta p (:114; k = 1: p = r + 0.0 r, :109), the owed x update (:127) and Ap = A p with the p.Ap level-1 values
    // (:123-125) in ONE launch: body k reads p_{k-1} in buffer (k - 1) & 1 and writes p_k into buffer k & 1
    const int which = k == 1;
    float* const pb[2] = { s->pf, s->pf2 };
    const sb_matrix* pm = s->A->fmt == 0 ? s->A->mirror : s->A; // (the latched plan: whatever mode the matrix is in by now)
    spmv_time_begin(s);
    launch_prog_fusep_f32(pm, s->A->fmt == 0, which ? s->rf : pb[(k - 1) & 1], s->rf, pb[k & 1], s->xf, s->Apf, s->SF, which, s->partialsF);
    spmv_time_end(s);
    mark(s, R_SPMVM);
    phase_mark(s, PH_SPMV);
    launch_sp_update_r(1, n, s->Apf, s->rf, s->SF, s->partials2F, stop, s->nPartials, s->partialsF, s->rrHistF, s->pApHistF);
    mark(s, R_WAXPBY);
    phase_mark(s, PH_R_UPDATE);
    sp_scalar<1>(s, s->partials2F, 1, 1); // the beta step / loop test: a launch of its own (the next SpMV's tiles all need beta)
    mark(s, R_DDOT);
    phase_mark(s, PH_BETA);
    return;
  }
  if (halo_fold_plan(s)) {
    // the halo exchange inside the loop's own kernels (sbhip_cg.inc.h: halo_fold_plan): p update + push | SpMV whose halo blocks
    // wait and read the staging area (+ p.Ap level 1) | alpha | r update (+ r.r level 1) | beta -- 5 launches
    sb_halo* h         = s->halo;
    const int which    = k == 1;
    const uint32_t vb  = 1024u;
    const dim3 gridV(sp_update_p_grid(n)), blockV(vb); // (cg_update_p_f32's grid: the plan's owner map follows it)
    const HaloFold& hf = halo_fold_send_plan(h, 1, gridV.x, vb);
    const unsigned long long seq = ++h->seq;
    hipLaunchKernelGGL(cg_update_p_push_f32, gridV, blockV, 0, g.stream, h->push, hf, seq, n, (const float*)s->rf, s->pf,
        which ? (float*)nullptr : s->xf, s->SF, which);
    HIP_CHECK(hipGetLastError());
    mark(s, R_WAXPBY);
    phase_mark(s, PH_P_UPDATE);
    uint32_t perI = 0, gridS = 0;
    const ScsHalo hh = halo_fold_spmv_arg(h, s->A, seq, &s->SF->stop, &perI, &gridS);
    const sb_matrix* m = s->A;
    spmv_time_begin(s);
    SB_SPMV_LAUNCH(spmv_scs64_halo_f32, dim3(gridS), dim3(256), 0, g.stream, m->chunkPtr, m->chunkLens, m->colInd, m->valf,
        (const float*)s->pf, s->Apf, m->nr, m->nChunks, perI, s->partialsF, stop, hh);
    HIP_CHECK(hipGetLastError());
    spmv_time_end(s);
    mark(s, R_SPMVM);
    phase_mark(s, PH_SPMV);
    sp_alpha_r_beta(s);
    return;
  }
  if (k == 1) { // p = r + 0.0 r (:109)
    launch_sp_update_p(0, n, s->rf, s->pf, nullptr, s->SF, 1, 0u, nullptr, nullptr);
  } else if (s->fused) { // beta step at the head, p = r + beta p, the owed x += alpha p (:111-116, :127)
    launch_sp_update_p(s->betaFold ? 1 : 0, n, s->rf, s->pf, s->xf, s->SF, 0, s->nPartials, s->partials2F, s->rrHistF);
    s->betaFold = 0;
  } else { // rtrans = r.r ; beta ; p = r + beta p (:111-114)
    sp_dot(s, s->rf, s->rf, stop);
    phase_mark(s, PH_DOT_PASS);
    sp_scalar<1>(s, s->partialsF, 0, 0);
    mark(s, R_DDOT);
    phase_mark(s, PH_BETA);
    launch_sp_update_p(0, n, s->rf, s->pf, nullptr, s->SF, 0, 0u, nullptr, nullptr);
  }
  mark(s, R_WAXPBY);
  phase_mark(s, PH_P_UPDATE);
  if (multi_rank() && s->halo) { // commExchange(&comm, p) (:122)
    halo_exchange_f32(s->halo, s->pf, stop, true);
    mark(s, R_COMM);
    phase_mark(s, PH_HALO);
  }
  // Ap = A p (:123) and p.Ap (:124-125)
  const bool fusedDot = s->fused && sp_spmv_has_dot(s);
  spmv_time_begin(s);
  launch_spmv_f32(s->A, s->pf, s->Apf, fusedDot ? s->partialsF : nullptr, stop);
  spmv_time_end(s);
  mark(s, R_SPMVM);
  phase_mark(s, PH_SPMV);
  if (s->fused) {
    if (!fusedDot && n) {
      launch_sp_dot_l1(n, s->pf, s->Apf, s->partialsF, stop);
      phase_mark(s, PH_DOT_PASS);
    }
    // alpha (:126) inside the r update: r = r - alpha Ap (:128) + the level-1 values of the next r.r; x += alpha p is owed
    if (multi_rank()) { // the all-reduced alpha step, r update, the all-reduced beta step / loop test (x += alpha p stays owed)
      sp_alpha_r_beta(s);
      return;
    }
    launch_sp_update_r(1, n, s->Apf, s->rf, s->SF, s->partials2F, stop, s->nPartials, s->partialsF, s->rrHistF, s->pApHistF);
    mark(s, R_WAXPBY);
    phase_mark(s, PH_R_UPDATE);
    s->betaFold = 1; // the beta step / loop test rides at the head of the next p update (sp_flush_beta where none follows)
    return;
  }
  sp_dot(s, s->pf, s->Apf, stop);
  phase_mark(s, PH_DOT_PASS);
  sp_scalar<2>(s, s->partialsF, 0, 0);
  mark(s, R_DDOT);
  phase_mark(s, PH_ALPHA);
  if (n) { // x = x + alpha p ; r = r + (-alpha) Ap (:127-128)
    launch_sp_axpy_sdev(n, s->xf, &s->SF->alpha, s->pf, s->xf, stop);
    launch_sp_axpy_sdev(n, s->rf, &s->SF->neg_alpha, s->Apf, s->rf, stop);
    mark(s, R_WAXPBY);
    phase_mark(s, PH_R_UPDATE);
  }
}

static void sp_cg_start(sb_cg* s, int itermax, double eps)
{
  const uint32_t n = s->nr;
  s->started    = false;
  s->seqLatched = -1;
  s->seqLatched = cg_seq(s) ? 1 : 0;
  apply_dot_order(s);
  s->fusepLatched = sp_fusep_plan(s) ? 1 : 0; // decided once per solve (sp_fusep_plan)
  s->foldLatched  = -1;
  s->foldLatched  = halo_fold_plan(s) ? 1 : 0; // ... and so is the folded halo exchange (sbhip_cg.inc.h: halo_fold_plan)
  if (s->fusepLatched && !s->pf2) s->pf2 = (float*)sb_malloc((size_t)s->nc * sizeof(float));
  if (itermax + 2 > s->hist_cap) {
    sb_free(s->rrHistF), sb_free(s->pApHistF);
    s->hist_cap = itermax + 2;
    s->rrHistF  = (float*)sb_malloc((size_t)s->hist_cap * sizeof(float));
    s->pApHistF = (float*)sb_malloc((size_t)s->hist_cap * sizeof(float));
  }
  s->timing = !s->fused;
  s->evUsed = 0;
  CgScalarsF h;
  memset(&h, 0, sizeof h);
  h.itermax = itermax, h.eps = (float)eps, h.hist_cap = s->hist_cap; // CG_FLOAT eps = (CG_FLOAT)param->eps (:64)
  HIP_CHECK(hipStreamSynchronize(g.stream));
  HIP_CHECK(hipMemcpy(s->SF, &h, sizeof h, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemset(s->XF, 0, sizeof(CgCommF)));
  halo_push_watch(s->halo, &s->XF->p2p_error, true);
  HIP_CHECK(hipMemsetAsync(s->xf, 0, (size_t)n * sizeof(float), g.stream)); // x0 = 0 (:28)
  HIP_CHECK(hipMemsetAsync(s->pf, 0, (size_t)s->nc * sizeof(float), g.stream));
  if (s->pf2) HIP_CHECK(hipMemsetAsync(s->pf2, 0, (size_t)s->nc * sizeof(float), g.stream));
  mark(s, -1);
  // prologue, src/CGSolver.c:94-100: p = x + 0.0 x ; Ap = A p ; r = b + (-1.0) Ap ; rtrans = r.r
  launch_sp_waxpby(n, 1.0f, s->xf, 0.0f, s->xf, s->pf, nullptr);
  mark(s, R_WAXPBY);
  halo_exchange_f32(s->halo, s->pf, nullptr, false); // (:96)
  mark(s, R_COMM);
  launch_spmv_f32(s->A, s->pf, s->Apf, nullptr, nullptr);
  mark(s, R_SPMVM);
  launch_sp_waxpby(n, 1.0f, s->bf, -1.0f, s->Apf, s->rf, nullptr);
  mark(s, R_WAXPBY);
  sp_dot(s, s->rf, s->rf, nullptr);
  sp_scalar<0>(s, s->partialsF, 0, 0);
  mark(s, R_DDOT);
  s->k_next = 1, s->started = true, s->betaFold = 0;
}

static void sp_cg_run_iters(sb_cg* s, int iters)
{
  phase_mark(s, -1);
  for (int i = 0; i < iters; i++) sp_loop_body(s, s->k_next++);
  sp_flush_beta(s); // every call leaves the loop state complete
}

static int sp_cg_finish(sb_cg* s)
{
  if (s->nr) {
    // (fused p update: body k left p_k in buffer k & 1; which body ran last is on the device -- n_pAp -- not on the host)
    launch_sp_x_finalize(s->nr, s->xf, s->pf, sp_fusep_plan(s) ? s->pf2 : nullptr, s->SF);
    HIP_CHECK(hipMemsetAsync(&s->SF->x_pending, 0, sizeof(int), g.stream));
  }
  HIP_CHECK(hipStreamSynchronize(g.stream));
  CgScalarsF h;
  HIP_CHECK(hipMemcpy(&h, s->SF, sizeof h, hipMemcpyDeviceToHost));
  CgCommF x;
  HIP_CHECK(hipMemcpy(&x, s->XF, sizeof x, hipMemcpyDeviceToHost));
  cg_comm_failures(s, x.p2p_error);
  cg_solve_over(s);
  return h.iters + 1;
}

static int sp_cg_history(const sb_cg* s, double* rr_out, int rr_cap, double* pAp_out, int pAp_cap, int* n_pAp)
{ // the float values, exactly, in the double arrays of sb_cg_history
  HIP_CHECK(hipStreamSynchronize(g.stream));
  CgScalarsF h;
  HIP_CHECK(hipMemcpy(&h, s->SF, sizeof h, hipMemcpyDeviceToHost));
  int nrr = std::min(std::min(h.n_rr, s->hist_cap), rr_cap), npa = std::min(std::min(h.n_pAp, s->hist_cap), pAp_cap);
  std::vector<float> t((size_t)std::max(std::max(nrr, npa), 1));
  if (nrr > 0) HIP_CHECK(hipMemcpy(t.data(), s->rrHistF, (size_t)nrr * sizeof(float), hipMemcpyDeviceToHost));
  for (int i = 0; i < nrr; i++) rr_out[i] = (double)t[i];
  if (npa > 0) HIP_CHECK(hipMemcpy(t.data(), s->pApHistF, (size_t)npa * sizeof(float), hipMemcpyDeviceToHost));
  for (int i = 0; i < npa; i++) pAp_out[i] = (double)t[i];
  if (n_pAp) *n_pAp = std::max(npa, 0);
  return std::max(nrr, 0);
}

static void sp_cg_counters(const sb_cg* s, int out[5])
{
  HIP_CHECK(hipStreamSynchronize(g.stream));
  CgScalarsF h;
  HIP_CHECK(hipMemcpy(&h, s->SF, sizeof h, hipMemcpyDeviceToHost));
  out[0] = h.stop, out[1] = h.stop_next, out[2] = h.iters, out[3] = h.n_rr, out[4] = h.n_pAp;
}

void sb_cg_solution_f32(const sb_cg* s, float* x_host)
{
  need_init();
  if (s->prec != 1) SB_FATAL("sb_cg_solution_f32 on a double-precision solver: use sb_cg_solution");
  float* tmp = sp_scratch(1, s->nr);
  sb_unpermute_f32(s->A, s->xf, tmp);
  sb_d2h(x_host, tmp, (size_t)s->nr * sizeof(float));
}

static double sp_cg_check_residual(const sb_cg* s)
{
  if (!s->xexactf || s->nr == 0) return 0.0;
  const uint32_t blocks = stream_grid(s->nr, 256);
  float* q              = reinterpret_cast<float*>(scratch_partials(blocks));
  hipLaunchKernelGGL(max_abs_diff_f32_k, dim3(blocks), dim3(256), 0, g.stream, s->nr, (const float*)s->xf,
      (const float*)s->xexactf, q);
  HIP_CHECK(hipGetLastError());
  std::vector<float> h(blocks);
  sb_d2h(h.data(), q, blocks * sizeof(float));
  float m = 0.0f;
  for (float v : h)
    if (v > m) m = v;
  if (multi_rank()) { // commReduction(&residual, MAX), src/CGSolver.c:55
    float* d = reinterpret_cast<float*>(g.scalar);
    sb_h2d(d, &m, sizeof m);
    sb_comm_reduction_f32(d, 0);
    sb_d2h(&m, d, sizeof m);
  }
  return (double)m;
}

// --- blocking test entries: the SP loop's vector and scalar kernels alone, launched by the loop's own launch functions (DESIGN
// 4.4.1; the fp64 twins are at the end of sbhip_cg.inc.h) ----------------------------------------------------------------------
void sb_cg_update_p_launch_f32(uint32_t n, uint32_t out[3])
{
  need_init();
  out[0] = sp_update_p_grid(n), out[1] = 1024u, out[2] = (uint32_t)g.prop.multiProcessorCount;
}
void sb_cg_update_r_launch_f32(uint32_t n, uint32_t out[3])
{
  need_init();
  out[0] = sp_groups_grid(n, 1), out[1] = 1024u, out[2] = (uint32_t)g.prop.multiProcessorCount;
}
void sb_dot_l1_launch_f32(uint32_t n, uint32_t out[3])
{
  need_init();
  out[0] = sp_groups_grid(n, 2), out[1] = 1024u, out[2] = (uint32_t)g.prop.multiProcessorCount;
}
void sb_stream_launch_f32(uint32_t n, uint32_t out[3])
{
  need_init();
  out[0] = stream_grid(n, 256), out[1] = 256u, out[2] = (uint32_t)g.prop.multiProcessorCount;
}

namespace {
enum { SP_BLK_GUARD = 64 }; // guard words (8 bytes each) in front of a payload and behind it
// `bytes` of plain host data (a multiple of 8) on the device between two runs of guard words
struct SpGuarded {
  std::vector<unsigned long long> up;
  char* raw = nullptr;
  size_t words;
  SpGuarded(const void* payload, size_t bytes) : words(bytes / 8)
  {
    up.resize(2 * SP_BLK_GUARD + words);
    for (size_t k = 0; k < up.size(); k++) up[k] = 0x7FF8C0DE00000000ull | k; // quiet NaNs with a payload, as doubles and as floats
    memcpy(&up[SP_BLK_GUARD], payload, bytes);
    raw = (char*)sb_malloc(up.size() * 8);
    HIP_CHECK(hipStreamSynchronize(g.stream));
    HIP_CHECK(hipMemcpy(raw, up.data(), up.size() * 8, hipMemcpyHostToDevice));
  }
  void* ptr() const { return raw + 8 * SP_BLK_GUARD; }
  // waits for the launch; the payload back into `out`; returns the number of guard words that changed
  int done(void* out)
  {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(g.stream));
    std::vector<unsigned long long> back(up.size());
    HIP_CHECK(hipMemcpy(back.data(), raw, back.size() * 8, hipMemcpyDeviceToHost));
    sb_free(raw);
    int changed = 0;
    for (size_t k = 0; k < back.size(); k++)
      if ((k < SP_BLK_GUARD || k >= back.size() - SP_BLK_GUARD) && back[k] != up[k]) changed++;
    memcpy(out, &back[SP_BLK_GUARD], words * 8);
    return changed;
  }
};
// The control block of a test entry: the caller's plain data (include/sbhip.h: blk_f[7], blk_beta[1], blk_i[10]) as a
// CgScalarsF between guard words, every field copied back behind the launch.  Nothing in between is computed here.
struct SpTestBlock {
  static CgScalarsF pack(const float* f, const double* beta, const int* i)
  {
    static_assert(sizeof(CgScalarsF) % 8 == 0, "the guard words follow the block without a gap");
    CgScalarsF h = zeroed<CgScalarsF>();
    h.rr = f[0], h.rr_old = f[1], h.pAp = f[2], h.alpha = f[3], h.neg_alpha = f[4], h.eps = f[5], h.snap_rr = f[6];
    memcpy(&h.beta, beta, sizeof h.beta); // (bits, not values: a NaN keeps its payload)
    h.stop = i[0], h.stop_next = i[1], h.iters = i[2], h.n_rr = i[3], h.n_pAp = i[4], h.itermax = i[5], h.hist_cap = i[6];
    h.x_pending = i[7], h.snap_iters = i[8], h.snap_stop_next = i[9];
    return h;
  }
  CgScalarsF h;
  SpGuarded dev;
  CgScalarsF* S;
  SpTestBlock(const float* f, const double* beta, const int* i) : h(pack(f, beta, i)), dev(&h, sizeof h), S((CgScalarsF*)dev.ptr()) {}
  int done(float* f, double* beta, int* i)
  {
    const int changed = dev.done(&h);
    f[0] = h.rr, f[1] = h.rr_old, f[2] = h.pAp, f[3] = h.alpha, f[4] = h.neg_alpha, f[5] = h.eps, f[6] = h.snap_rr;
    memcpy(beta, &h.beta, sizeof h.beta);
    i[0] = h.stop, i[1] = h.stop_next, i[2] = h.iters, i[3] = h.n_rr, i[4] = h.n_pAp, i[5] = h.itermax, i[6] = h.hist_cap;
    i[7] = h.x_pending, i[8] = h.snap_iters, i[9] = h.snap_stop_next;
    return changed;
  }
};
// a stop flag of its own on the device, between guard words
struct SpTestFlag {
  int h[2];
  SpGuarded dev;
  SpTestFlag(int stopped) : h{ stopped, 0 }, dev(h, sizeof h) {}
  const int* flag() const { return (const int*)dev.ptr(); }
  int done()
  {
    const int was = h[0];
    const int changed = dev.done(h);
    return changed + (h[0] != was || h[1] != 0 ? 1 : 0); // (the kernels only read it)
  }
};
void sp_need_mode(int mode, int top, const char* fn)
{
  if (mode < 0 || mode > top) SB_FATAL("%s: mode = %d outside 0 .. %d", fn, mode, top);
}
} // namespace

int sb_cg_update_p_native_f32(int mode, uint32_t n, const float* r_dev, float* p_dev, float* x_dev, int which, uint32_t m,
    const float* l1_dev, float* rr_hist_dev, float* blk_f, double* blk_beta, int* blk_i)
{
  need_init();
  sp_need_mode(mode, 1, "sb_cg_update_p_native_f32");
  if (mode && which) SB_FATAL("sb_cg_update_p_native_f32: mode 1 takes which = 0 only");
  need_aligned16({ r_dev, p_dev, x_dev }, "sb_cg_update_p_native_f32", "vectors");
  SpTestBlock b(blk_f, blk_beta, blk_i);
  launch_sp_update_p(mode, n, r_dev, p_dev, x_dev, b.S, which, m, l1_dev, rr_hist_dev);
  return b.done(blk_f, blk_beta, blk_i);
}

int sb_cg_update_r_native_f32(int mode, uint32_t n, const float* Ap_dev, float* r_dev, float* l1out_dev, uint32_t m,
    const float* l1in_dev, float* rr_hist_dev, float* pAp_hist_dev, float* blk_f, double* blk_beta, int* blk_i)
{
  need_init();
  sp_need_mode(mode, 1, "sb_cg_update_r_native_f32");
  need_aligned16({ Ap_dev, r_dev }, "sb_cg_update_r_native_f32", "vectors");
  SpTestBlock b(blk_f, blk_beta, blk_i);
  launch_sp_update_r(mode, n, Ap_dev, r_dev, b.S, l1out_dev, &b.S->stop, m, l1in_dev, rr_hist_dev, pAp_hist_dev);
  return b.done(blk_f, blk_beta, blk_i);
}

int sb_cg_scalar_native_f32(int mode, int split, uint32_t m, const float* q_dev, float* rr_hist_dev, float* pAp_hist_dev, int defer_x,
    int l1, float* blk_f, double* blk_beta, int* blk_i, float* local)
{
  need_init();
  sp_need_mode(mode, 2, "sb_cg_scalar_native_f32");
  if (split < 0 || split > 2) SB_FATAL("sb_cg_scalar_native_f32: split = %d outside 0 .. 2", split);
  SpTestBlock b(blk_f, blk_beta, blk_i);
  if (split == 0) {
    launch_sp_scalar(mode, m, q_dev, b.S, rr_hist_dev, pAp_hist_dev, defer_x, l1);
    return b.done(blk_f, blk_beta, blk_i);
  }
  CgCommF x = zeroed<CgCommF>();
  x.local   = *local;
  static_assert(sizeof(CgCommF) == 8, "one guarded word");
  SpGuarded X(&x, sizeof x);
  if (split == 1) launch_sp_local(m, q_dev, b.S, (CgCommF*)X.ptr(), l1);
  else launch_sp_apply_local(mode, b.S, (const CgCommF*)X.ptr(), rr_hist_dev, pAp_hist_dev, defer_x);
  int changed = b.done(blk_f, blk_beta, blk_i);
  changed += X.done(&x);
  if (x.p2p_error != 0) changed++; // (neither kernel writes it)
  *local = x.local;
  return changed;
}

int sb_cg_x_finalize_native_f32(uint32_t n, float* x_dev, const float* p0_dev, const float* p1_dev, float* blk_f, double* blk_beta,
    int* blk_i)
{
  need_init();
  SpTestBlock b(blk_f, blk_beta, blk_i);
  launch_sp_x_finalize(n, x_dev, p0_dev, p1_dev, b.S);
  return b.done(blk_f, blk_beta, blk_i);
}

int sb_axpy_sdev_native_f32(uint32_t n, const float* x_dev, int negative, const float* y_dev, float* w_dev, float* blk_f,
    double* blk_beta, int* blk_i)
{
  need_init();
  SpTestBlock b(blk_f, blk_beta, blk_i);
  launch_sp_axpy_sdev(n, x_dev, negative ? &b.S->neg_alpha : &b.S->alpha, y_dev, w_dev, &b.S->stop);
  return b.done(blk_f, blk_beta, blk_i);
}

int sb_dot_l1_native_f32(uint32_t n, const float* a_dev, const float* b_dev, float* l1out_dev, int stopped)
{
  need_init();
  need_aligned16({ a_dev, b_dev }, "sb_dot_l1_native_f32", "vectors");
  SpTestFlag f(stopped);
  launch_sp_dot_l1(n, a_dev, b_dev, l1out_dev, f.flag());
  return f.done();
}

int sb_waxpby_stop_native_f32(uint32_t n, float alpha, const float* x_dev, float beta, const float* y_dev, float* w_dev, int stopped)
{
  need_init();
  SpTestFlag f(stopped);
  launch_sp_waxpby(n, alpha, x_dev, beta, y_dev, w_dev, f.flag());
  return f.done();
}
