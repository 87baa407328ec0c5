// sbhip_mg.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): the one plan of
// PCG's preconditioners behind the diagonal, and the one V-cycle that makes z = M^-1 r from it (kernels:
// mg.hip.h, mg_fw.hip.h, mg_poly.hip.h).  A plan is levels, a smoother (the sweeps of sbhip_sgs.inc.h or the polynomial of
// sbhip_poly.inc.h) and a transfer between the levels; the sweeps alone and the polynomial alone are its one-level cases.  What
// builds the plans is sbhip_mg_fw.inc.h's (a caller's prolongations) and sbhip_precond.inc.h's (the entry points); the loop and
// every other sb_pcg_* call are sbhip_pcg.inc.h's and sbhip_pcg_loop.inc.h's.
// ===========================================================================
// the preconditioner plan and its V-cycle
// ===========================================================================
enum PrecondSmoother { SMOOTH_SGS, SMOOTH_CHEB };
enum PrecondTransfer { TRANSFER_NONE, TRANSFER_INJECT, TRANSFER_FW };

// the injection to the next level: Sell-64 over the next level's rows in its device order
struct MgInject {
  uint32_t nRChunks = 0;
  SellRows R = {};             // device arrays: the stored non-zero entries of the fine rows that are coarse points
  uint32_t* fineRow = nullptr; // per slot of R its fine device row: also the translated f2c the prolongation uses
  double restrictBytes = 0.0;
};
// the full-weighting transfers to the next level
struct MgFw {
  SellRows PT = {}, Pm = {}; // omega P^T over the next level's rows, P over this level's; device arrays
  uint32_t nPTChunks = 0, nPChunks = 0;
  double omega = 0.0;
  double transferBytes = 0.0;           // both structures as one cycle reads them
  double *diag = nullptr, *d = nullptr; // under the sweeps: the diagonal whose reciprocal is dinv, the full residual
};
// of the smoother's and the transfer's members a level fills those the plan names; the others stay empty
struct PrecondLevel {
  const sb_matrix* A = nullptr;
  uint32_t n = 0;
  double* dinv = nullptr;            // level 0: the handle's own
  sb_halo* halo = nullptr;           // level 0 of a several-rank handle: fills z's halo tail ahead of every SpMV
  double *r = nullptr, *z = nullptr; // levels 1 ..: the restricted residual and the correction (level 0: the caller's)
  SgsPlan* sgs = nullptr;            // SMOOTH_SGS
  struct {
    PolyCoef c;                        // this level's interval and coefficients; c.steps: `steps`, on the last level `coarseSteps`
    double *d = nullptr, *w = nullptr; // the recurrence's direction and A z
  } cheb;                            // SMOOTH_CHEB
  uint32_t nCoarse = 0;              // rows of the next level (absent on the last, as the transfers are)
  MgInject inj;                      // TRANSFER_INJECT
  MgFw fw;                           // TRANSFER_FW
};
struct PrecondPlan {
  int kind = 0; // as sb_pcg_precond reports it: 1 sweeps, 2 their cycle, 3 with full weighting, 4 polynomial, 5 its cycle
  PrecondSmoother smoother = SMOOTH_SGS;
  PrecondTransfer transfer = TRANSFER_NONE;
  std::vector<PrecondLevel> lev;
  int steps = 0, coarseSteps = 0; // SMOOTH_CHEB
  std::vector<double> g;          // kind 4: the bound's row values, device row order
};

namespace {
// the restriction structure of level l from its downloaded rows h and the injection map in original numbering
void mg_build_restrict(PrecondLevel& F, const sb_matrix* coarse, const HostRows& h, const uint32_t* f2c, int l)
{
  const uint32_t nf = F.n, ncs = coarse->nr;
  std::vector<uint32_t> seen(nf, 0);
  for (uint32_t c = 0; c < ncs; c++) {
    if (f2c[c] >= nf) SB_FATAL("sb_pcg_create_mg: f2c[%d][%u] = %u is outside the %u rows of level %d", l, c, f2c[c], nf, l);
    if (seen[f2c[c]]) SB_FATAL("sb_pcg_create_mg: f2c[%d][%u] = %u repeats entry %u: the coarse points must be distinct", l, c, f2c[c], seen[f2c[c]] - 1);
    seen[f2c[c]] = c + 1;
  }
  const std::vector<uint32_t> fo2n = old_to_device_rows(F.A), co2n = old_to_device_rows(coarse);
  MgInject& T = F.inj;
  F.nCoarse   = ncs;
  T.nRChunks  = (ncs + 63u) / 64u;
  std::vector<uint32_t> fineRow((size_t)T.nRChunks * 64u, 0xFFFFFFFFu);
  for (uint32_t c = 0; c < ncs; c++) fineRow[co2n[c]] = fo2n[f2c[c]];
  // (Sell padding is a stored +0.0 and drops out, as in sgs_build)
  auto stored = [&](uint32_t f, size_t q) {
    if (h.val[q] == 0.0) return false;
    if (h.col[q] >= nf) SB_FATAL("sb_pcg_create_mg: level %d: device row %u has column %u outside the %u rows", l, f, h.col[q], nf);
    return true;
  };
  std::vector<unsigned long long> chunkPtr;
  T.R       = sell64_pack(h, fineRow, stored, chunkPtr);
  T.fineRow = sgs_to_device(fineRow);
  // the structure with fineRow beside rowLen | per coarse row r and one gathered z in, rc out
  T.restrictBytes = sell64_bytes(chunkPtr[T.nRChunks], T.nRChunks, 8) + 24.0 * (double)ncs;
}
} // namespace

// steps 3 and 4 under the sweeps: d = r - A z over every row in one launch, rc = omega P^T d
static void mg_fw_restrict(const PrecondLevel& V, const double* r, const double* z, double* rc, const int* stop)
{
  const SgsPlan* P = V.sgs;
  if (P->nChunks)
    hipLaunchKernelGGL(mg_residual_k, dim3((P->nChunks + 3u) / 4u), dim3(256), 0, g.stream, P->nChunks, (const uint32_t*)P->rowIdx,
        P->half[0], P->half[1], r, z, (const double*)V.fw.diag, V.fw.d, stop);
  if (V.fw.nPTChunks)
    hipLaunchKernelGGL(mg_restrict_pt_k, dim3((V.fw.nPTChunks + 3u) / 4u), dim3(256), 0, g.stream, V.fw.nPTChunks, V.nCoarse, V.fw.PT,
        V.fw.omega, (const double*)V.fw.d, rc, stop);
}
// step 4 under the polynomial, behind w = A z: rc = omega P^T (r - w)
static void mgp_restrict(const PrecondLevel& V, const double* r, const double* w, double* rc, const int* stop)
{
  if (V.fw.nPTChunks)
    hipLaunchKernelGGL(mgp_restrict_k, dim3((V.fw.nPTChunks + 3u) / 4u), dim3(256), 0, g.stream, V.fw.nPTChunks, V.nCoarse, V.fw.PT,
        V.fw.omega, r, w, rc, stop);
}
// step 6: z = z + P zc
static void mg_fw_prolong(const PrecondLevel& V, const double* zc, double* z, const int* stop)
{
  if (V.fw.nPChunks)
    hipLaunchKernelGGL(mg_prolong_p_k, dim3((V.fw.nPChunks + 3u) / 4u), dim3(256), 0, g.stream, V.fw.nPChunks, V.fw.Pm, zc, z, stop);
}

// z = V(0, r) for every plan: r and z are level 0's vectors (the solve's, or sb_pcg_apply_precond's scratch), as are the
// sweeps' forward sums t there (the polynomial has none, and its z is an SpMV operand).  Down: smooth from zero, restrict the
// residual; up: prolong, smooth from the guess.  The polynomial's two hooks: firstDone, level 0's step 1 has been made by
// poly_update_r_k; l1rz != NULL, the kernel that finishes z leaves the level-1 values of r.z there (with one level and one step
// that kernel is the caller's poly_update_r_k)
static void precond_cycle(const PrecondPlan* M, const double* r, double* t, double* z, const int* stop, bool firstDone, double* l1rz)
{
  const size_t L = M->lev.size();
  for (size_t l = 0; l < L; l++) {
    const PrecondLevel& V = M->lev[l];
    if (!V.n) continue; // (an empty level is the last one, and the sweeps have no colour to launch on it)
    const double *rl = l ? V.r : r, *dinv = V.dinv;
    double* zl = l ? V.z : z;
    double* rc = l + 1 < L ? M->lev[l + 1].r : nullptr;
    switch (M->smoother) {
    case SMOOTH_SGS:
      sgs_apply(V.sgs, dinv, rl, l ? V.sgs->t : t, zl, stop);
      if (!rc) break;
      if (M->transfer == TRANSFER_FW) mg_fw_restrict(V, rl, zl, rc, stop);
      else if (V.inj.nRChunks)
        hipLaunchKernelGGL(mg_restrict_residual_k, dim3((V.inj.nRChunks + 3u) / 4u), dim3(256), 0, g.stream, V.inj.nRChunks,
            MgRestrict{ V.inj.R.chunkPtr, V.inj.R.chunkLen, V.inj.fineRow, V.inj.R.rowLen, V.inj.R.col, V.inj.R.val }, rl,
            (const double*)zl, rc, stop);
      break;
    case SMOOTH_CHEB:
      if (l || !firstDone)
        hipLaunchKernelGGL(poly_first_k, dim3(stream_grid(V.n, 256)), dim3(256), 0, g.stream, V.n, rl, dinv, V.cheb.d, zl, V.cheb.c.c1,
            stop);
      poly_steps(V.A, dinv, V.cheb.c, rl, zl, V.cheb.d, V.cheb.w, stop, L == 1 ? l1rz : nullptr, V.halo);
      if (!rc) break;
      launch_spmv(V.A, zl, V.cheb.w, nullptr, stop);
      mgp_restrict(V, rl, V.cheb.w, rc, stop);
      break;
    }
  }
  for (size_t l = L - 1; l-- > 0;) {
    const PrecondLevel& V = M->lev[l];
    if (!V.n) continue;
    const double *rl = l ? V.r : r, *dinv = V.dinv, *zc = M->lev[l + 1].z;
    double* zl = l ? V.z : z;
    if (M->transfer == TRANSFER_FW) mg_fw_prolong(V, zc, zl, stop);
    else if (V.nCoarse)
      hipLaunchKernelGGL(mg_prolong_add_k, dim3(stream_grid(V.nCoarse, 256)), dim3(256), 0, g.stream, V.nCoarse,
          (const uint32_t*)V.inj.fineRow, zc, zl, stop);
    switch (M->smoother) {
    case SMOOTH_SGS: sgs_apply_guess(V.sgs, dinv, rl, l ? V.sgs->t : t, zl, stop); break;
    case SMOOTH_CHEB: {
      double* lz = l ? nullptr : l1rz;
      launch_spmv(V.A, zl, V.cheb.w, nullptr, stop);
      mgp_first(V.n, rl, V.cheb.w, dinv, V.cheb.d, zl, V.cheb.c.c1, V.cheb.c.steps == 1 ? lz : nullptr, stop);
      poly_steps(V.A, dinv, V.cheb.c, rl, zl, V.cheb.d, V.cheb.w, stop, lz);
    } break;
    }
  }
  HIP_CHECK(hipGetLastError()); // (the sweeps' launches are checked here, once per cycle)
}

// launches of one cycle.  A smoothing from zero: 2 nC - 1 sweeps, or 2 steps - 1 (step 1, which in the loop is the r update's,
// then an SpMV and a step kernel per further step).  Per level but the last two smoothings, under the polynomial the SpMV ahead
// of the one from the guess, the residual (none of its own under injection), the restriction, the prolongation; the last level
// one smoothing
static int precond_cycle_launches(const PrecondPlan* M)
{
  const bool cheb = M->smoother == SMOOTH_CHEB;
  const int between = cheb ? 4 : M->transfer == TRANSFER_FW ? 3 : 2;
  const size_t L = M->lev.size();
  int n = 0;
  for (size_t l = 0; l < L; l++) {
    const int a = 2 * (cheb ? M->lev[l].cheb.c.steps : (int)M->lev[l].sgs->nC) - 1;
    n += l + 1 < L ? 2 * a + between : a;
  }
  return n;
}

// --- RightPrecond (sbhip_solver.inc.h): the cycle for the solvers that borrow it ------------------------------------------------
void RightPrecond::need_borrowable(const sb_matrix* m, const sb_pcg* M, const char* fn)
{
  if (!M) SB_FATAL("%s: no PCG handle to take the preconditioner from", fn);
  if (M->halo) SB_FATAL("%s: the PCG handle runs on several ranks; a solver that borrows its preconditioner runs on one rank", fn);
  if (M->A != m) SB_FATAL("%s: the PCG handle was made over another matrix: its preconditioner is that matrix's", fn);
  RightPrecond{ M }.need_closed(fn);
}
void RightPrecond::borrow(const sb_pcg* from, size_t bytes)
{
  if (from->pre) {
    M = from, plan = from->pre;
    return;
  }
  dinv = (double*)sb_malloc(bytes);
  if (from->nr) sb_d2d(dinv, from->dinv, (size_t)from->nr * sizeof(double));
}
void RightPrecond::need_closed(const char* fn) const
{
  if (M && M->clock.open)
    SB_FATAL("%s between sb_pcg_start and sb_pcg_finish of the borrowed PCG handle: the plan's vectors are in flight", fn);
}
int RightPrecond::kind() const { return plan ? plan->kind : 0; }
const double* RightPrecond::diagonal() const { return plan ? plan->lev[0].dinv : dinv; }
PrecondRide RightPrecond::ride() const
{
  if (!plan) return dinv ? PrecondRide{ 0, dinv, nullptr, 0.0 } : PrecondRide{};
  const PrecondLevel& V = plan->lev[0];
  return plan->smoother == SMOOTH_CHEB ? PrecondRide{ 1, V.dinv, V.cheb.d, V.cheb.c.c1 } : PrecondRide{};
}
void RightPrecond::apply(uint32_t n, const double* src, double* dst, const int* stop, bool rode) const
{
  if (!n) return;
  if (!plan) {
    if (rode) return;
    hipLaunchKernelGGL(precond_diag_k, dim3(stream_grid(n, 256)), dim3(256), 0, g.stream, n, src, (const double*)dinv, dst);
    HIP_CHECK(hipGetLastError());
    return;
  }
  if (!stop) stop = zero_flag(); // (the plan's kernels read their flag unconditionally)
  const bool cheb = plan->smoother == SMOOTH_CHEB;
  precond_cycle(plan, src, cheb ? nullptr : plan->lev[0].sgs->t, dst, stop, cheb && rode, nullptr);
}
// none for a diagonal, the cycle less level 0's step 1 under the polynomial, the whole cycle under the sweeps
int RightPrecond::apply_launches() const
{
  if (!plan) return 0;
  return precond_cycle_launches(plan) - (plan->smoother == SMOOTH_CHEB ? 1 : 0);
}

// bytes the full-weighting transfers of one level read and write beside their structures: P^T's gathered fine vectors in (d;
// r and w under the polynomial) and rc out; P's zc in, z in and out
static double mg_fw_vector_bytes(const PrecondLevel& V, int fineIn)
{
  return V.fw.transferBytes + 8.0 * fineIn * (double)V.n + 8.0 * (double)V.nCoarse + 8.0 * (double)V.nCoarse + 16.0 * (double)V.n;
}
// bytes one cycle reads and writes.  The sweeps: per level the smoothing from zero as sgs_bytes
// counts it; per level but the last the transfers (injection: the restriction structure with r and one gathered z in and rc out
// per coarse row, the prolongation's f2c, zc, z in, z out: 28 per coarse row; full weighting: the residual reads both halves of
// the sweep structure and r, z, diag per row and writes d) and the smoothing from the guess: forward both halves with r, dinv,
// one gathered z in and t, z out per row, backward as from zero.  The polynomial: per step behind the first the SpMV
// (sb_matrix_spmv_bytes) and poly_step_k's 56 B per row, step 1's dinv in, d and z out: 24; per level but the last twice that
// with two more SpMVs, mgp_first_k's 48 in the second step 1's place, and the transfers
static double precond_cycle_bytes(const PrecondPlan* M)
{
  double b       = 0.0;
  const size_t L = M->lev.size();
  for (size_t l = 0; l < L; l++) {
    const PrecondLevel& V = M->lev[l];
    const bool last       = l + 1 == L;
    const double n        = (double)V.n;
    if (M->smoother == SMOOTH_CHEB) {
      const double spmv = (double)sb_matrix_spmv_bytes(V.A), st = (double)V.cheb.c.steps;
      if (last) b += (st - 1.0) * (spmv + 56.0 * n) + 24.0 * n;
      else b += 2.0 * st * spmv + 2.0 * (st - 1.0) * 56.0 * n + 48.0 * n + 24.0 * n + mg_fw_vector_bytes(V, 2);
      continue;
    }
    const SgsPlan* P = V.sgs;
    b += sgs_bytes(P, V.n);
    if (last) break;
    if (M->transfer == TRANSFER_FW) b += P->halfBytes[0] + P->halfBytes[1] + 32.0 * n + mg_fw_vector_bytes(V, 1);
    else b += V.inj.restrictBytes + 28.0 * (double)V.nCoarse;
    b += P->halfBytes[0] + P->halfBytes[1] + 40.0 * n;                         // forward from the guess
    b += P->structBytes - P->halfBytes[0] + 32.0 * (double)P->rowsBackward;    // backward
  }
  return b;
}

static void precond_release(sb_pcg* s)
{
  PrecondPlan* M = s->pre;
  if (!M) return;
  for (size_t l = 0; l < M->lev.size(); l++) {
    PrecondLevel& V = M->lev[l];
    sgs_free_plan(V.sgs);
    sb_free(V.cheb.d), sb_free(V.cheb.w);
    sell64_free(V.inj.R), sb_free(V.inj.fineRow);
    sell64_free(V.fw.PT), sell64_free(V.fw.Pm), sb_free(V.fw.diag), sb_free(V.fw.d);
    if (l) sb_free(V.dinv), sb_free(V.r), sb_free(V.z); // level 0's are the handle's and the caller's
  }
  delete M;
  s->pre = nullptr;
}
