// sbhip_mg_fw.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): the second
// transfer mode of the multigrid V-cycle of sbhip_mg.inc.h (kernels: mg_fw.hip.h).  Per level but the last a
// prolongation P_l (n_l x n_{l+1}, the caller's CSR in original numbering on both sides) and the restriction omega_l P_l^T of the
// FULL residual stand in for the injection.  The levels, the smoother, the handle and the loop are sbhip_mg.inc.h's.
// ===========================================================================
// full-weighting transfers
// ===========================================================================

// every refusal of level l's prolongation, before anything is built
static void mg_fw_check(const char* fn, const MgFwArgs& a, int l, uint32_t nFine, uint32_t nCoarseRows)
{
  const uint64_t* ptr = a.ptr[l];
  if (!(a.omega[l] > 0.0) || !std::isfinite(a.omega[l]))
    SB_FATAL("%s: omega[%d] = %g: the restriction's scale of level %d must be finite and positive", fn, l, a.omega[l], l);
  for (uint32_t i = 0; i < nFine; i++)
    if (ptr[i + 1] < ptr[i])
      SB_FATAL("%s: level %d: the prolongation's row pointer falls from %llu to %llu at row %u", fn, l, (unsigned long long)ptr[i],
          (unsigned long long)ptr[i + 1], i);
  for (uint32_t i = 0; i < nFine; i++)
    for (uint64_t q = ptr[i]; q < ptr[i + 1]; q++) {
      if (a.col[l][q] >= nCoarseRows)
        SB_FATAL("%s: level %d: the prolongation's row %u has column %u outside the %u rows of level %d", fn, l, i, a.col[l][q],
            nCoarseRows, l + 1);
      if (!std::isfinite(a.val[l][q]))
        SB_FATAL("%s: level %d: the prolongation's row %u has a weight that is not finite (column %u)", fn, l, i, a.col[l][q]);
    }
}

namespace {
// a transfer's kept entries (HostRows over its device rows, a row's entries in the order the contract sums them) -> Sell-64,
// slot == device row
SellRows mg_fw_sell(const HostRows& R, uint32_t* nChunksOut, double* bytes)
{
  const uint32_t n = (uint32_t)R.ptr.size() - 1u, nChunks = (n + 63u) / 64u;
  std::vector<uint32_t> slotRow((size_t)nChunks * 64u, 0xFFFFFFFFu);
  for (uint32_t d = 0; d < n; d++) slotRow[d] = d;
  std::vector<unsigned long long> chunkPtr;
  const SellRows T = sell64_pack(R, slotRow, [](uint32_t, size_t) { return true; }, chunkPtr);
  *nChunksOut = nChunks;
  *bytes += sell64_bytes(chunkPtr[nChunks], nChunks, 4);
  return T;
}
} // namespace

// level l's two structures from its (checked) prolongation: P in this level's device order with the next level's device rows
// as columns, entries in the caller's storage order; P^T the other way round, a coarse row's entries in ascending ORIGINAL fine
// row number (equal rows: storage order).  A stored weight of 0.0 is dropped from both
static void mg_fw_transfers(MgLevel& F, const sb_matrix* coarse, const MgFwArgs& a, int l)
{
  const uint32_t nf = F.n, ncs = coarse->nr;
  const std::vector<uint32_t> fo2n = old_to_device_rows(F.A), co2n = old_to_device_rows(coarse);
  HostRows p, pt;
  p.ptr.assign((size_t)nf + 1, 0), pt.ptr.assign((size_t)ncs + 1, 0);
  for (uint32_t i = 0; i < nf; i++)
    for (uint64_t q = a.ptr[l][i]; q < a.ptr[l][i + 1]; q++)
      if (a.val[l][q] != 0.0) p.ptr[(size_t)fo2n[i] + 1]++, pt.ptr[(size_t)co2n[a.col[l][q]] + 1]++;
  for (uint32_t d = 0; d < nf; d++) p.ptr[d + 1] += p.ptr[d];
  for (uint32_t d = 0; d < ncs; d++) pt.ptr[d + 1] += pt.ptr[d];
  p.col.resize(p.ptr[nf]), p.val.resize(p.ptr[nf]), pt.col.resize(pt.ptr[ncs]), pt.val.resize(pt.ptr[ncs]);
  {
    // original fine rows ascending: a row of P fills in storage order, a row of P^T in ascending original fine row
    std::vector<size_t> nextT(pt.ptr.begin(), pt.ptr.end() - 1);
    for (uint32_t i = 0; i < nf; i++) {
      size_t o = p.ptr[fo2n[i]];
      for (uint64_t q = a.ptr[l][i]; q < a.ptr[l][i + 1]; q++) {
        const double w = a.val[l][q];
        if (w == 0.0) continue;
        const uint32_t cd = co2n[a.col[l][q]];
        p.col[o] = cd, p.val[o] = w, o++;
        pt.col[nextT[cd]] = fo2n[i], pt.val[nextT[cd]] = w, nextT[cd]++;
      }
    }
  }
  F.nCoarse = ncs;
  F.omega   = a.omega[l];
  F.PT      = mg_fw_sell(pt, &F.nPTChunks, &F.transferBytes);
  F.Pm      = mg_fw_sell(p, &F.nPChunks, &F.transferBytes);
}
// ... and the level's diagonal and d, which the full residual needs
static void mg_fw_build(MgLevel& F, const sb_matrix* coarse, const MgFwArgs& a, int l)
{
  mg_fw_transfers(F, coarse, a, l);
  const size_t nb = (size_t)F.n * sizeof(double) + 4096;
  F.diag = (double*)sb_malloc(nb), F.d = (double*)sb_malloc(nb);
  launch_diagonal(F.A, F.diag, nullptr);
  HIP_CHECK(hipStreamSynchronize(g.stream));
}

static void mg_fw_free(MgLevel& V)
{
  sell64_free(V.PT), sell64_free(V.Pm);
  sb_free(V.diag), sb_free(V.d);
  V.diag = V.d = nullptr;
}

// steps 3 and 4: d = r - A z over every row in one launch, rc = omega P^T d
static void mg_fw_restrict(const MgLevel& V, const double* r, const double* z, double* rc, const int* stop)
{
  const SgsPlan* P = V.P;
  if (P->nChunks)
    hipLaunchKernelGGL(mg_residual_k, dim3((P->nChunks + 3u) / 4u), dim3(256), 0, g.stream, P->nChunks, (const uint32_t*)P->rowIdx,
        P->half[0], P->half[1], r, z, (const double*)V.diag, V.d, stop);
  if (V.nPTChunks)
    hipLaunchKernelGGL(mg_restrict_pt_k, dim3((V.nPTChunks + 3u) / 4u), dim3(256), 0, g.stream, V.nPTChunks, V.nCoarse, V.PT, V.omega,
        (const double*)V.d, rc, stop);
}
// step 6: z = z + P zc
static void mg_fw_prolong(const MgLevel& V, const double* zc, double* z, const int* stop)
{
  if (V.nPChunks)
    hipLaunchKernelGGL(mg_prolong_p_k, dim3((V.nPChunks + 3u) / 4u), dim3(256), 0, g.stream, V.nPChunks, V.Pm, zc, z, stop);
}

// bytes the transfers of one level read and write: the residual reads both halves of the sweep structure and r, z, diag per
// row and writes d; the restriction reads its structure and d and writes rc; the prolongation its structure and zc, z in and out
static double mg_fw_bytes(const MgLevel& V)
{
  return V.P->halfBytes[0] + V.P->halfBytes[1] + 32.0 * (double)V.n // the residual
         + V.transferBytes + 8.0 * (double)V.n + 8.0 * (double)V.nCoarse // P^T, d in, rc out
         + 8.0 * (double)V.nCoarse + 16.0 * (double)V.n;                // P (counted above), zc in, z in and out
}

sb_pcg* sb_pcg_create_mg_p(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int nCoarse,
    const sb_matrix* const* coarse, const uint64_t* const* p_ptr, const uint32_t* const* p_col, const double* const* p_val,
    const double* omega)
{
  const MgFwArgs a = { p_ptr, p_col, p_val, omega };
  return mg_create("sb_pcg_create_mg_p", m, halo, b_host, xexact_host, nCoarse, coarse, nullptr, &a);
}

// steps 3, 4 and 6 on level l alone, on scratch vectors: d and rc from (r, z), z_out = z after prolonging zc.  r, z, d_out and
// z_out in level l's original row order, zc and rc_out in level l + 1's
void sb_pcg_mg_fw_probe(sb_pcg* s, int l, const double* r_host, const double* z_host, const double* zc_host, double* d_out,
    double* rc_out, double* z_out)
{
  need_init();
  if (!s->mg || !s->mg->fw) SB_FATAL("sb_pcg_mg_fw_probe: the handle has no full-weighting transfers (sb_pcg_create_mg_p makes them)");
  if (s->clock.open) SB_FATAL("sb_pcg_mg_fw_probe between sb_pcg_start and sb_pcg_finish: the solve's vectors are in flight");
  const int L = (int)s->mg->lev.size();
  if (l < 0 || l + 1 >= L) SB_FATAL("sb_pcg_mg_fw_probe: level %d of a handle with %d levels has no transfers", l, L);
  MgLevel V        = s->mg->lev[l]; // a copy: its d is the probe's own
  const MgLevel& C = s->mg->lev[l + 1];
  const size_t nf = (size_t)V.n * sizeof(double) + 4096, nc = (size_t)C.n * sizeof(double) + 4096;
  double *r = (double*)sb_malloc(nf), *z = (double*)sb_malloc(nf), *d = (double*)sb_malloc(nf);
  double *zc = (double*)sb_malloc(nc), *rc = (double*)sb_malloc(nc);
  upload_permuted(V.A, r_host, r), upload_permuted(V.A, z_host, z), upload_permuted(C.A, zc_host, zc);
  V.d = d;
  mg_fw_restrict(V, r, z, rc, zero_flag());
  mg_fw_prolong(V, zc, z, zero_flag());
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(g.stream));
  download_original(V.A, d, d_out), download_original(C.A, rc, rc_out), download_original(V.A, z, z_out);
  sb_free(r), sb_free(z), sb_free(d), sb_free(zc), sb_free(rc);
}
