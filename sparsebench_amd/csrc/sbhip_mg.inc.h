// sbhip_mg.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): HPCG's
// preconditioner, a geometric multigrid V-cycle with the multicolour symmetric Gauss-Seidel smoother of sbhip_sgs.inc.h
// (kernels: mg.hip.h).  The handle is an sb_pcg whose `mg` plan is set and whose `sgs` plan is level 0's smoother:
// the loop and every other sb_pcg_* call are sbhip_pcg.inc.h's and sbhip_sgs.inc.h's; what differs is how z is made.
// ===========================================================================
// multigrid V-cycle
// ===========================================================================
struct MgLevel {
  const sb_matrix* A = nullptr;
  uint32_t n = 0;
  SgsPlan* P = nullptr;   // level 0: the handle's own `sgs`
  double* dinv = nullptr; // level 0: the handle's own
  double *r = nullptr, *z = nullptr; // levels 1 ..: the restricted residual and the correction (level 0: the caller's)
  // the restriction to the next level (absent on the last): Sell-64 over its rows in its device order
  uint32_t nCoarse = 0, nRChunks = 0;
  SellRows R = {};             // device arrays: the stored non-zero entries of the fine rows that are coarse points
  uint32_t* fineRow = nullptr; // per slot of R its fine device row: also the translated f2c the prolongation uses
  double restrictBytes = 0.0;
  // the full-weighting transfers to the next level (sbhip_mg_fw.inc.h) in the injection's place
  double *diag = nullptr, *d = nullptr; // the diagonal whose reciprocal is dinv; the full residual
  SellRows PT = {}, Pm = {};            // omega P^T over the next level's rows, P over this level's; device arrays
  uint32_t nPTChunks = 0, nPChunks = 0;
  double omega = 0.0;
  double transferBytes = 0.0;           // both structures as one cycle reads them
};
struct MgPlan {
  std::vector<MgLevel> lev;
  bool fw = false; // full-weighting transfers (sb_pcg_create_mg_p) in place of injection
};
// (sbhip_mg_fw.inc.h) a caller's prolongations: their checks, the structures of one level, the transfers' launches and bytes
struct MgFwArgs {
  const uint64_t* const* ptr;
  const uint32_t* const* col;
  const double* const* val;
  const double* omega;
};
static void mg_fw_check(const char* fn, const MgFwArgs& a, int l, uint32_t nFine, uint32_t nCoarseRows);
static void mg_fw_transfers(MgLevel& F, const sb_matrix* coarse, const MgFwArgs& a, int l);
static void mg_fw_build(MgLevel& F, const sb_matrix* coarse, const MgFwArgs& a, int l);
static void mg_fw_free(MgLevel& V);
static void mg_fw_restrict(const MgLevel& V, const double* r, const double* z, double* rc, const int* stop);
static void mg_fw_prolong(const MgLevel& V, const double* zc, double* z, const int* stop);
static double mg_fw_bytes(const MgLevel& V);

namespace {
// the restriction structure of level l from its downloaded rows h and the injection map in original numbering
void mg_build_restrict(MgLevel& F, const sb_matrix* coarse, const HostRows& h, const uint32_t* f2c, int l)
{
  const uint32_t nf = F.n, ncs = coarse->nr;
  std::vector<uint32_t> seen(nf, 0);
  for (uint32_t c = 0; c < ncs; c++) {
    if (f2c[c] >= nf) SB_FATAL("sb_pcg_create_mg: f2c[%d][%u] = %u is outside the %u rows of level %d", l, c, f2c[c], nf, l);
    if (seen[f2c[c]]) SB_FATAL("sb_pcg_create_mg: f2c[%d][%u] = %u repeats entry %u: the coarse points must be distinct", l, c, f2c[c], seen[f2c[c]] - 1);
    seen[f2c[c]] = c + 1;
  }
  const std::vector<uint32_t> fo2n = old_to_device_rows(F.A), co2n = old_to_device_rows(coarse);
  F.nCoarse  = ncs;
  F.nRChunks = (ncs + 63u) / 64u;
  std::vector<uint32_t> fineRow((size_t)F.nRChunks * 64u, 0xFFFFFFFFu);
  for (uint32_t c = 0; c < ncs; c++) fineRow[co2n[c]] = fo2n[f2c[c]];
  // (Sell padding is a stored +0.0 and drops out, as in sgs_build)
  auto stored = [&](uint32_t f, size_t q) {
    if (h.val[q] == 0.0) return false;
    if (h.col[q] >= nf) SB_FATAL("sb_pcg_create_mg: level %d: device row %u has column %u outside the %u rows", l, f, h.col[q], nf);
    return true;
  };
  std::vector<unsigned long long> chunkPtr;
  F.R       = sell64_pack(h, fineRow, stored, chunkPtr);
  F.fineRow = sgs_to_device(fineRow);
  // the structure with fineRow beside rowLen | per coarse row r and one gathered z in, rc out
  F.restrictBytes = sell64_bytes(chunkPtr[F.nRChunks], F.nRChunks, 8) + 24.0 * (double)ncs;
}
} // namespace

static void mg_release(sb_pcg* s)
{
  MgPlan* M = s->mg;
  if (!M) return;
  for (size_t l = 0; l < M->lev.size(); l++) {
    MgLevel& V = M->lev[l];
    sell64_free(V.R), sb_free(V.fineRow);
    mg_fw_free(V);
    if (l == 0) continue; // level 0's smoother, dinv, r and z are the handle's
    sgs_free_plan(V.P);
    sb_free(V.dinv), sb_free(V.r), sb_free(V.z);
  }
  delete M;
  s->mg = nullptr;
}

// the forward sweep from the guess in z (both halves of the plan, t kept), then the smoother's own backward sweep
static void mg_post_smooth(const SgsPlan* P, const double* dinv, const double* r, double* t, double* z, const int* stop)
{
  for (uint32_t c = 0; c < P->nC; c++)
    hipLaunchKernelGGL(mg_sweep_guess_k, sgs_grid(P, c), dim3(256), 0, g.stream, P->chunk0[c], P->chunk0[c + 1] - P->chunk0[c],
        (const uint32_t*)P->rowIdx, P->half[0], P->half[1], r, dinv, t, z, stop);
  sgs_backward(P, dinv, t, z, stop);
}

// z = V(0, r): r, t and z are level 0's vectors (the solve's, or sb_pcg_apply_precond's scratch)
static void mg_apply(const sb_pcg* s, const double* r, double* t, double* z, const int* stop)
{
  const MgPlan* M = s->mg;
  const size_t L  = M->lev.size();
  // down: pre-smooth from zero, the residual at the coarse points
  for (size_t l = 0; l < L; l++) {
    const MgLevel& V   = M->lev[l];
    const double* rl   = l ? V.r : r;
    double *tl = l ? V.P->t : t, *zl = l ? V.z : z;
    sgs_apply(V.P, (const double*)V.dinv, rl, tl, zl, stop);
    if (l + 1 < L && M->fw) mg_fw_restrict(V, rl, zl, M->lev[l + 1].r, stop);
    else if (l + 1 < L && V.nRChunks)
      hipLaunchKernelGGL(mg_restrict_residual_k, dim3((V.nRChunks + 3u) / 4u), dim3(256), 0, g.stream, V.nRChunks,
          MgRestrict{ V.R.chunkPtr, V.R.chunkLen, V.fineRow, V.R.rowLen, V.R.col, V.R.val }, rl, (const double*)zl, M->lev[l + 1].r, stop);
  }
  // up: prolong, post-smooth from the guess
  for (size_t l = L - 1; l-- > 0;) {
    const MgLevel& V = M->lev[l];
    const double* rl = l ? V.r : r;
    double *tl = l ? V.P->t : t, *zl = l ? V.z : z;
    if (M->fw) mg_fw_prolong(V, M->lev[l + 1].z, zl, stop);
    else if (V.nCoarse)
      hipLaunchKernelGGL(mg_prolong_add_k, dim3(stream_grid(V.nCoarse, 256)), dim3(256), 0, g.stream, V.nCoarse, (const uint32_t*)V.fineRow,
          (const double*)M->lev[l + 1].z, zl, stop);
    mg_post_smooth(V.P, (const double*)V.dinv, rl, tl, zl, stop);
  }
  HIP_CHECK(hipGetLastError());
}

// launches of one V-cycle: per level but the last two smoothing applies (2 nC - 1 each), the restriction (full weighting: the
// residual and the restriction), the prolongation; the last level one apply
static int mg_apply_launches(const sb_pcg* s)
{
  int n = 0;
  const size_t L = s->mg->lev.size();
  for (size_t l = 0; l < L; l++) {
    const int a = 2 * (int)s->mg->lev[l].P->nC - 1;
    n += l + 1 < L ? 2 * a + (s->mg->fw ? 3 : 2) : a;
  }
  return n;
}

// bytes one V-cycle reads and writes: per level the pre-smoothing apply as sgs_bytes counts it; per level but the
// last the restriction structure with r and one gathered z in and rc out per coarse row, the prolongation (f2c, zc, z in, z out:
// 28 per coarse row), and the post-smoothing: forward both halves of the sweep structure with r, dinv, one gathered z in and t, z
// out per row, backward as the apply's
static double mg_bytes(const sb_pcg* s)
{
  double b = 0.0;
  const size_t L = s->mg->lev.size();
  for (size_t l = 0; l < L; l++) {
    const MgLevel& V = s->mg->lev[l];
    b += sgs_bytes(V.P, V.n);
    if (l + 1 == L) break;
    b += s->mg->fw ? mg_fw_bytes(V) : V.restrictBytes + 28.0 * (double)V.nCoarse;
    b += V.P->halfBytes[0] + V.P->halfBytes[1] + 40.0 * (double)V.n;                    // forward from the guess
    b += V.P->structBytes - V.P->halfBytes[0] + 32.0 * (double)V.P->rowsBackward;       // backward
  }
  return b;
}

// every refusal of a caller's hierarchy, before anything is built.  fn: the entry point as messages name it.  fw NULL: injection
// by f2c_host; else its prolongations (f2c_host NULL)
static void mg_check_hierarchy(const char* fn, const sb_matrix* m, int nCoarse, const sb_matrix* const* coarse,
    const uint32_t* const* f2c_host, const MgFwArgs* fw)
{
  if (nCoarse < 0) SB_FATAL("%s: nCoarse = %d: the number of coarse levels cannot be negative", fn, nCoarse);
  if (nCoarse > 0 && (!coarse || (fw ? !fw->ptr || !fw->col || !fw->val || !fw->omega : !f2c_host)))
    SB_FATAL("%s: %d coarse levels need their matrices and %s", fn, nCoarse, fw ? "prolongations" : "injection maps");
  // every level is looked at before anything is built (level 0 here for its shape alone: pcg_create would take its extra
  // columns for another rank's and say so)
  if (m->nr != m->nc) SB_FATAL("%s: the matrix of level 0 is not square (%u rows, %u columns)", fn, m->nr, m->nc);
  for (int l = 1; l <= nCoarse; l++) {
    const sb_matrix* c    = coarse[l - 1];
    const sb_matrix* fine = l == 1 ? m : coarse[l - 2];
    if (!c || (fw ? !fw->ptr[l - 1] || !fw->col[l - 1] || !fw->val[l - 1] : !f2c_host[l - 1]))
      SB_FATAL("%s: level %d has no matrix or no %s", fn, l, fw ? "prolongation from it" : "injection map");
    if (c->prec != 2) SB_FATAL("%s: MG: double precision only (the matrix of level %d was uploaded in single precision)", fn, l);
    if (c->nr != c->nc) SB_FATAL("%s: the matrix of level %d is not square (%u rows, %u columns)", fn, l, c->nr, c->nc);
    if (c->nr >= fine->nr)
      SB_FATAL("%s: level %d has %u rows, level %d has %u: every level must be smaller than the one above it", fn, l, c->nr, l - 1,
          fine->nr);
  }
  if (fw)
    for (int l = 0; l < nCoarse; l++) mg_fw_check(fn, *fw, l, l ? coarse[l - 1]->nr : m->nr, coarse[l]->nr);
}

// fn, f2c_host, fw: as mg_check_hierarchy takes them
static sb_pcg* mg_create(const char* fn, const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int nCoarse,
    const sb_matrix* const* coarse, const uint32_t* const* f2c_host, const MgFwArgs* fw)
{
  need_init();
  mg_check_hierarchy(fn, m, nCoarse, coarse, f2c_host, fw);
  char who[64];
  snprintf(who, sizeof who, "MG (level %d)", 0);
  sb_pcg* s = pcg_create(m, halo, b_host, xexact_host, nullptr, fn, who);
  MgPlan* M = new MgPlan();
  M->lev.resize((size_t)nCoarse + 1);
  M->fw = fw != nullptr;
  s->mg = M;
  for (int l = 0; l <= nCoarse; l++) {
    MgLevel& V = M->lev[l];
    V.A = l ? coarse[l - 1] : m;
    V.n = V.A->nr;
    if (l) {
      const size_t nb = (size_t)V.n * sizeof(double) + 4096;
      V.dinv = (double*)sb_malloc(nb), V.r = (double*)sb_malloc(nb), V.z = (double*)sb_malloc(nb);
      snprintf(who, sizeof who, "MG (level %d)", l);
      jacobi_dinv(V.A, V.dinv, fn, who);
    } else {
      V.dinv = s->dinv;
    }
    HostRows h = sgs_download(V.A); // once: the restriction reads the rows whole, the smoother's plan compacts them
    if (l < nCoarse && fw) mg_fw_build(V, coarse[l], *fw, l);
    else if (l < nCoarse) mg_build_restrict(V, coarse[l], h, f2c_host[l], l);
    snprintf(who, sizeof who, "%s: level %d", fn, l);
    V.P = sgs_build(V.A, std::move(h), who);
    if (!l) s->sgs = V.P;
  }
  HIP_CHECK(hipStreamSynchronize(g.stream));
  return s;
}

sb_pcg* sb_pcg_create_mg(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int nCoarse,
    const sb_matrix* const* coarse, const uint32_t* const* f2c_host)
{
  return mg_create("sb_pcg_create_mg", m, halo, b_host, xexact_host, nCoarse, coarse, f2c_host, nullptr);
}

// (sbhip_mg_poly.inc.h) the levels of a Chebyshev-smoothed cycle, which has no SgsPlan: no colours
static int mgp_levels(const sb_pcg* s);
static uint32_t mgp_level_rows(const sb_pcg* s, int l);

int sb_pcg_levels(const sb_pcg* s) { return s->mgp ? mgp_levels(s) : s->mg ? (int)s->mg->lev.size() : s->sgs ? 1 : 0; }
static const SgsPlan* mg_level_plan(const sb_pcg* s, int l, const char* fn)
{
  if (l < 0 || l >= sb_pcg_levels(s)) SB_FATAL("%s: level %d of a handle with %d levels", fn, l, sb_pcg_levels(s));
  return s->mg ? s->mg->lev[l].P : s->sgs;
}
uint32_t sb_pcg_level_rows(const sb_pcg* s, int l)
{
  mg_level_plan(s, l, "sb_pcg_level_rows");
  return s->mgp ? mgp_level_rows(s, l) : s->mg ? s->mg->lev[l].n : s->nr;
}
int sb_pcg_level_colours(const sb_pcg* s, int l)
{
  const SgsPlan* P = mg_level_plan(s, l, "sb_pcg_level_colours");
  return P ? (int)P->nC : 0;
}
