// sbhip_mg_fw.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): the
// full-weighting transfers between the levels of a preconditioner plan (sbhip_mg.inc.h) as a caller gives them (DESIGN 4.14;
// kernels: mg_fw.hip.h): per level but the last a prolongation P_l (n_l x n_{l+1}, the caller's CSR in original numbering on both
// sides) and the restriction omega_l P_l^T of the FULL residual.  Here: their checks, the structures built from them, and the
// probes that run one level's transfers alone.  Their launches are the cycle's, in sbhip_mg.inc.h.
// ===========================================================================
// full-weighting transfers
// ===========================================================================
struct MgFwArgs {
  const uint64_t* const* ptr;
  const uint32_t* const* col;
  const double* const* val;
  const double* omega;
};

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
static void mg_fw_transfers(PrecondLevel& F, const sb_matrix* coarse, const MgFwArgs& a, int l)
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
  F.nCoarse  = ncs;
  F.fw.omega = a.omega[l];
  F.fw.PT    = mg_fw_sell(pt, &F.fw.nPTChunks, &F.fw.transferBytes);
  F.fw.Pm    = mg_fw_sell(p, &F.fw.nPChunks, &F.fw.transferBytes);
}
// ... and under the sweeps the level's diagonal and d, which the full residual needs
static void mg_fw_build(PrecondLevel& F, const sb_matrix* coarse, const MgFwArgs& a, int l)
{
  mg_fw_transfers(F, coarse, a, l);
  const size_t nb = (size_t)F.n * sizeof(double) + 4096;
  F.fw.diag = (double*)sb_malloc(nb), F.fw.d = (double*)sb_malloc(nb);
  launch_diagonal(F.A, F.fw.diag, nullptr);
  HIP_CHECK(hipStreamSynchronize(g.stream));
}

namespace {
// The two probes run the transfers of level l alone on scratch vectors of their own: three of level l's rows, two of level
// l + 1's, in the levels' original row order on the host.  A NULL host vector is neither uploaded nor downloaded
struct ProbeVecs {
  const sb_matrix *F, *C;
  double *f[3], *c[2];
};
ProbeVecs probe_upload(const PrecondLevel& V, const PrecondLevel& C, const double* const (&f_host)[3], const double* const (&c_host)[2])
{
  ProbeVecs p = { V.A, C.A, {}, {} };
  for (int i = 0; i < 3; i++) {
    p.f[i] = (double*)sb_malloc((size_t)V.n * sizeof(double) + 4096);
    if (f_host[i]) upload_permuted(p.F, f_host[i], p.f[i]);
  }
  for (int i = 0; i < 2; i++) {
    p.c[i] = (double*)sb_malloc((size_t)C.n * sizeof(double) + 4096);
    if (c_host[i]) upload_permuted(p.C, c_host[i], p.c[i]);
  }
  return p;
}
void probe_download(ProbeVecs& p, double* const (&f_out)[3], double* const (&c_out)[2])
{
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(g.stream));
  for (int i = 0; i < 3; i++) {
    if (f_out[i]) download_original(p.F, p.f[i], f_out[i]);
    sb_free(p.f[i]);
  }
  for (int i = 0; i < 2; i++) {
    if (c_out[i]) download_original(p.C, p.c[i], c_out[i]);
    sb_free(p.c[i]);
  }
}
} // namespace

// steps 3, 4 and 6 on level l alone: d and rc from (r, z), z_out = z after prolonging zc.  r, z, d_out and z_out in level l's
// original row order, zc and rc_out in level l + 1's
void sb_pcg_mg_fw_probe(sb_pcg* s, int l, const double* r_host, const double* z_host, const double* zc_host, double* d_out,
    double* rc_out, double* z_out)
{
  need_init();
  if (!s->pre || s->pre->kind != 3)
    SB_FATAL("sb_pcg_mg_fw_probe: the handle has no full-weighting transfers (sb_pcg_create_mg_p makes them)");
  if (s->clock.open) SB_FATAL("sb_pcg_mg_fw_probe between sb_pcg_start and sb_pcg_finish: the solve's vectors are in flight");
  const int L = (int)s->pre->lev.size();
  if (l < 0 || l + 1 >= L) SB_FATAL("sb_pcg_mg_fw_probe: level %d of a handle with %d levels has no transfers", l, L);
  PrecondLevel V = s->pre->lev[l]; // a copy: its d is the probe's own
  ProbeVecs p    = probe_upload(V, s->pre->lev[l + 1], { r_host, z_host, nullptr }, { zc_host, nullptr });
  V.fw.d         = p.f[2];
  mg_fw_restrict(V, p.f[0], p.f[1], p.c[1], zero_flag());
  mg_fw_prolong(V, p.c[0], p.f[1], zero_flag());
  probe_download(p, { nullptr, z_out, d_out }, { nullptr, rc_out });
}

// steps 4 and 6 of the Chebyshev-smoothed cycle on level l alone: rc = omega P^T (r - w), z_out = z after prolonging zc.  r, w,
// z and z_out in level l's original row order, zc and rc_out in level l + 1's
void sb_pcg_mg_poly_probe(sb_pcg* s, int l, const double* r_host, const double* w_host, const double* z_host, const double* zc_host,
    double* rc_out, double* z_out)
{
  need_init();
  const char* fn = "sb_pcg_mg_poly_probe";
  if (!s->pre || s->pre->kind != 5)
    SB_FATAL("%s: the handle has another preconditioner (sb_pcg_create_mg_poly makes the Chebyshev-smoothed cycle)", fn);
  if (s->clock.open) SB_FATAL("%s between sb_pcg_start and sb_pcg_finish: the solve's vectors are in flight", fn);
  const int L = (int)s->pre->lev.size();
  if (l < 0 || l + 1 >= L) SB_FATAL("%s: level %d of a handle with %d levels has no transfers", fn, l, L);
  const PrecondLevel& V = s->pre->lev[l];
  ProbeVecs p           = probe_upload(V, s->pre->lev[l + 1], { r_host, w_host, z_host }, { zc_host, nullptr });
  mgp_restrict(V, p.f[0], p.f[1], p.c[1], zero_flag());
  mg_fw_prolong(V, p.c[0], p.f[2], zero_flag());
  probe_download(p, { nullptr, nullptr, z_out }, { nullptr, rc_out });
}
