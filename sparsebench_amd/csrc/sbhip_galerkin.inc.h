// sbhip_galerkin.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): the
// Galerkin coarse operator A_c = P^T A P formed on the device (kernels: galerkin.hip.h).  Set-up work: nothing here
// runs inside a solver's loop.  The matrix is read in place from the reference-layout arrays of its upload; P comes as the
// caller's CSR in original numbering on both sides (as sb_pcg_create_mg_p takes it); the result lives on the host.
// ===========================================================================
// Galerkin product
// ===========================================================================
struct sb_csr {
  uint32_t n = 0;
  std::vector<uint64_t> ptr;
  std::vector<uint32_t> col;
  std::vector<double> val;
  double stats[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
};

namespace {
// a product's output on the device: 64-bit row pointers, ascending columns, sums
struct GalOut {
  uint64_t* ptr = nullptr;
  uint32_t* col = nullptr;
  double* val   = nullptr;
  uint64_t nnz  = 0;
  uint32_t maxRow = 0;
  double ms       = 0.0; // both launches
};
void gal_free(GalOut& o) { sb_free(o.ptr), sb_free(o.col), sb_free(o.val), o = GalOut(); }

void gal_need_bytes(const char* gal_fn, int stage, const char* what, double bytes)
{
  const double have = (double)sb_mem_free_bytes();
  if (bytes > have)
    SB_FATAL("%s: stage %d: %s needs %.0f bytes of device memory, %.0f are free", gal_fn, stage, what, bytes, have);
}

// C = X Y, stage 1 (SKIPY: a stored weight of 0.0 in Y has no term) or 2; gal_fn: the entry point the messages name
template <class X, bool SKIPY> GalOut gal_product(const char* gal_fn, int stage, uint32_t nRows, const X& x, const GalMap& map, const GalY& y)
{
  GalOut o;
  std::vector<uint64_t> ptr((size_t)nRows + 1, 0);
  if (nRows == 0) {
    o.ptr = sgs_to_device(ptr);
    return o;
  }
  gal_need_bytes(gal_fn, stage, "the row counts and pointers", 12.0 * (double)nRows + 64.0);
  uint32_t* count = (uint32_t*)sb_malloc((size_t)nRows * sizeof(uint32_t));
  unsigned long long* flags = (unsigned long long*)sb_malloc(16); // [0] the first row above the capacity, [1] bad columns
  const unsigned long long init[2] = { ~0ull, 0ull };
  sb_h2d(flags, init, sizeof init);
  unsigned int* bad = (unsigned int*)(flags + 1);
  hipEvent_t ev[4];
  for (hipEvent_t& e : ev) HIP_CHECK(hipEventCreate(&e));
  HIP_CHECK(hipEventRecord(ev[0], g.stream));
  hipLaunchKernelGGL((gal_count_k<X, SKIPY>), dim3(nRows), dim3(64), 0, g.stream, nRows, x, map, y, count, flags, bad);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(ev[1], g.stream));
  std::vector<uint32_t> cnt(nRows);
  sb_d2h(cnt.data(), count, (size_t)nRows * sizeof(uint32_t));
  unsigned long long got[2];
  sb_d2h(got, flags, sizeof got);
  sb_free(count);
  if (got[1] & 1ull)
    SB_FATAL("%s: stage %d: an entry of the left factor has a column outside the %u rows of the right one", gal_fn, stage, y.nY);
  if (got[0] != ~0ull)
    SB_FATAL("%s: stage %d (%s): row %u has at least %u distinct columns, the capacity of a row is %u: refused, not "
             "truncated", gal_fn, stage, stage == 1 ? "A P" : "P^T (A P)", (uint32_t)(got[0] >> 32), (uint32_t)(got[0] & 0xFFFFFFFFull), GAL_CAP);
  for (uint32_t i = 0; i < nRows; i++) ptr[i + 1] = ptr[i] + cnt[i], o.maxRow = std::max(o.maxRow, cnt[i]);
  o.nnz = ptr[nRows];
  gal_need_bytes(gal_fn, stage, "the product", 12.0 * (double)o.nnz + 8.0 * (double)nRows + 64.0);
  o.ptr = sgs_to_device(ptr);
  o.col = (uint32_t*)sb_malloc((size_t)o.nnz * sizeof(uint32_t)), o.val = (double*)sb_malloc((size_t)o.nnz * sizeof(double));
  HIP_CHECK(hipEventRecord(ev[2], g.stream));
  hipLaunchKernelGGL((gal_fill_k<X, SKIPY>), dim3(nRows), dim3(64), 0, g.stream, nRows, x, map, y, (const uint64_t*)o.ptr, o.col, o.val, bad);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(ev[3], g.stream));
  sb_d2h(got, flags, sizeof got);
  sb_free(flags);
  if (got[1]) SB_FATAL("%s: stage %d: the second pass found other rows than the first (flags %llu)", gal_fn, stage, got[1]);
  float a = 0.f, b = 0.f;
  HIP_CHECK(hipEventElapsedTime(&a, ev[0], ev[1]));
  HIP_CHECK(hipEventElapsedTime(&b, ev[2], ev[3]));
  for (hipEvent_t& e : ev) HIP_CHECK(hipEventDestroy(e));
  o.ms = (double)a + (double)b;
  return o;
}

// stage 1 alone: T = A Y with A read in place in its device order, T in the original numbering of both sides; Y has A's rows
GalOut gal_stage1(const char* fn, const sb_matrix* A, const GalY& y)
{
  const bool perm   = A->fmt == 1 && A->permuted;
  const GalMap mapA = { perm ? A->oldToNew : nullptr, perm ? A->newToOld : nullptr };
  return A->fmt == 0 ? gal_product<GalCrs, true>(fn, 1, A->nr, GalCrs{ A->rowPtr, A->colInd, A->val }, mapA, y)
                     : gal_product<GalSell, true>(fn, 1, A->nr, GalSell{ A->chunkPtr, A->chunkLens, A->C, A->colInd, A->val }, mapA, y);
}
} // namespace

sb_csr* sb_matrix_galerkin(const sb_matrix* A, uint32_t nCoarse, const uint64_t* p_ptr, const uint32_t* p_col, const double* p_val)
{
  need_init();
  const char* fn = "sb_matrix_galerkin";
  if (!A || !p_ptr || !p_col || !p_val) SB_FATAL("%s: no matrix or no prolongation", fn);
  if (A->prec != 2) SB_FATAL("%s: double precision only (the matrix was uploaded in single precision)", fn);
  if (A->nr != A->nc)
    SB_FATAL("%s: the matrix is not square (%u rows, %u columns: halo columns of several ranks are not supported)", fn, A->nr, A->nc);
  const uint32_t n = A->nr;
  {
    const double one = 1.0;
    const MgFwArgs a = { &p_ptr, &p_col, &p_val, &one };
    mg_fw_check(fn, a, 0, n, nCoarse);
  }
  if (p_ptr[0] != 0) SB_FATAL("%s: the prolongation's row pointer starts at %llu, not 0", fn, (unsigned long long)p_ptr[0]);
  for (uint32_t i = 0; i < n; i++)
    if (p_ptr[i + 1] - p_ptr[i] > (1ull << 24))
      SB_FATAL("%s: the prolongation's row %u has %llu entries (at most %llu)", fn, i, (unsigned long long)(p_ptr[i + 1] - p_ptr[i]), 1ull << 24);
  const uint64_t nnzP = p_ptr[n];
  // P^T over the coarse rows: a row's kept entries in ascending original fine row, equal rows in storage order (mg_fw_transfers')
  std::vector<uint64_t> tptr((size_t)nCoarse + 1, 0);
  for (uint64_t q = 0; q < nnzP; q++)
    if (p_val[q] != 0.0) tptr[(size_t)p_col[q] + 1]++;
  for (uint32_t c = 0; c < nCoarse; c++) tptr[c + 1] += tptr[c];
  std::vector<uint32_t> tcol(tptr[nCoarse]);
  std::vector<double> tval(tptr[nCoarse]);
  {
    std::vector<uint64_t> next(tptr.begin(), tptr.end() - 1);
    for (uint32_t i = 0; i < n; i++)
      for (uint64_t q = p_ptr[i]; q < p_ptr[i + 1]; q++)
        if (p_val[q] != 0.0) tcol[next[p_col[q]]] = i, tval[next[p_col[q]]] = p_val[q], next[p_col[q]]++;
  }
  gal_need_bytes(fn, 1, "the prolongation and its transpose", 24.0 * (double)nnzP + 8.0 * ((double)n + (double)nCoarse) + 4096.0);

  // stage 1: T = A P, A in place in its device order, T in the original numbering of both sides
  uint64_t* dPptr = (uint64_t*)sb_malloc(((size_t)n + 1) * sizeof(uint64_t));
  uint32_t* dPcol = (uint32_t*)sb_malloc((size_t)nnzP * sizeof(uint32_t));
  double* dPval   = (double*)sb_malloc((size_t)nnzP * sizeof(double));
  sb_h2d(dPptr, p_ptr, ((size_t)n + 1) * sizeof(uint64_t));
  if (nnzP) sb_h2d(dPcol, p_col, (size_t)nnzP * sizeof(uint32_t)), sb_h2d(dPval, p_val, (size_t)nnzP * sizeof(double));
  const GalY yP = { dPptr, dPcol, dPval, n };
  GalOut T      = gal_stage1(fn, A, yP);
  sb_free(dPptr), sb_free(dPcol), sb_free(dPval);

  // stage 2: A_c = P^T T
  uint64_t* dTptr = sgs_to_device(tptr);
  uint32_t* dTcol = sgs_to_device(tcol);
  double* dTval   = sgs_to_device(tval);
  const GalY yT   = { T.ptr, T.col, T.val, n };
  GalOut R        = gal_product<GalCsr64, false>(fn, 2, nCoarse, GalCsr64{ dTptr, dTcol, dTval }, GalMap{ nullptr, nullptr }, yT);
  sb_free(dTptr), sb_free(dTcol), sb_free(dTval);

  // download; an entry whose sum compares equal to 0.0 is dropped (NaN is kept)
  sb_csr* c = new sb_csr();
  c->n      = nCoarse;
  std::vector<uint64_t> rptr((size_t)nCoarse + 1);
  std::vector<uint32_t> rcol(R.nnz);
  std::vector<double> rval(R.nnz);
  sb_d2h(rptr.data(), R.ptr, rptr.size() * sizeof(uint64_t));
  if (R.nnz) sb_d2h(rcol.data(), R.col, (size_t)R.nnz * sizeof(uint32_t)), sb_d2h(rval.data(), R.val, (size_t)R.nnz * sizeof(double));
  c->ptr.assign((size_t)nCoarse + 1, 0);
  c->col.reserve(R.nnz), c->val.reserve(R.nnz);
  for (uint32_t r = 0; r < nCoarse; r++) {
    for (uint64_t q = rptr[r]; q < rptr[r + 1]; q++)
      if (!(rval[q] == 0.0)) c->col.push_back(rcol[q]), c->val.push_back(rval[q]);
    c->ptr[r + 1] = c->col.size();
  }
  c->stats[0] = T.ms, c->stats[1] = R.ms, c->stats[2] = (double)T.nnz, c->stats[3] = (double)(R.nnz - c->col.size());
  c->stats[4] = (double)T.maxRow, c->stats[5] = (double)R.maxRow;
  gal_free(T), gal_free(R);
  return c;
}

uint32_t sb_csr_rows(const sb_csr* c) { return c->n; }
uint64_t sb_csr_nnz(const sb_csr* c) { return c->ptr[c->n]; }
void sb_csr_copy(const sb_csr* c, uint64_t* ptr, uint32_t* col, double* val)
{
  memcpy(ptr, c->ptr.data(), c->ptr.size() * sizeof(uint64_t));
  if (!c->col.empty()) memcpy(col, c->col.data(), c->col.size() * sizeof(uint32_t)), memcpy(val, c->val.data(), c->val.size() * sizeof(double));
}
void sb_csr_stats(const sb_csr* c, double out[6])
{
  for (int i = 0; i < 6; i++) out[i] = c->stats[i];
}
void sb_csr_free(sb_csr* c) { delete c; }
