// sbhip_precond.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): the entry
// points that make a PCG handle with a preconditioner plan (sbhip_mg.inc.h), and the queries that read it.
// The handle is an sb_pcg whose `pre` is set: the loop, its control block, histories and every other sb_pcg_* call are
// sbhip_pcg.inc.h's and sbhip_pcg_loop.inc.h's.
// ===========================================================================
// preconditioner plans: creation and queries
// ===========================================================================

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

// a handle whose plan has the levels' matrices and nothing else yet; level 0's dinv is the handle's.
// who: the preconditioner as the diagonal's refusal names it; ranksOk: as pcg_create takes it
static sb_pcg* precond_create(const char* fn, const char* who, int kind, const sb_matrix* m, sb_halo* halo, const double* b_host,
    const double* xexact_host, int nCoarse, const sb_matrix* const* coarse, bool ranksOk = false)
{
  sb_pcg* s      = pcg_create(m, halo, b_host, xexact_host, nullptr, fn, who, ranksOk);
  PrecondPlan* M = new PrecondPlan();
  M->kind        = kind;
  M->lev.resize((size_t)nCoarse + 1);
  for (int l = 0; l <= nCoarse; l++) M->lev[l].A = l ? coarse[l - 1] : m, M->lev[l].n = M->lev[l].A->nr;
  M->lev[0].dinv = s->dinv;
  s->pre         = M;
  return s;
}
// dinv, r and z of a level below the first.  who: as precond_create takes it.  zOperand: z is an SpMV operand, as p is (nc
// entries and the kernels' padding, zeroed)
static void precond_level_vectors(PrecondLevel& V, const char* fn, const char* who, bool zOperand)
{
  const size_t nb = (size_t)V.n * sizeof(double) + 4096, nz = zOperand ? (size_t)V.A->nc * sizeof(double) + 4096 : nb;
  V.dinv = (double*)sb_malloc(nb), V.r = (double*)sb_malloc(nb), V.z = (double*)sb_malloc(nz);
  if (zOperand) HIP_CHECK(hipMemsetAsync(V.z, 0, nz, g.stream));
  jacobi_dinv(V.A, V.dinv, fn, who);
}

// the sweeps alone: a cycle of one level
sb_pcg* sb_pcg_create_sgs(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host)
{
  const char* fn = "sb_pcg_create_sgs";
  sb_pcg* s      = precond_create(fn, "SGS", 1, m, halo, b_host, xexact_host, 0, nullptr);
  s->pre->lev[0].sgs = sgs_build(m, sgs_download(m), fn);
  HIP_CHECK(hipStreamSynchronize(g.stream));
  return s;
}

// fn, f2c_host, fw: as mg_check_hierarchy takes them
static sb_pcg* mg_create(const char* fn, const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int nCoarse,
    const sb_matrix* const* coarse, const uint32_t* const* f2c_host, const MgFwArgs* fw)
{
  need_init();
  mg_check_hierarchy(fn, m, nCoarse, coarse, f2c_host, fw);
  char who[64];
  snprintf(who, sizeof who, "MG (level %d)", 0);
  sb_pcg* s      = precond_create(fn, who, fw ? 3 : 2, m, halo, b_host, xexact_host, nCoarse, coarse);
  PrecondPlan* M = s->pre;
  M->transfer    = fw ? TRANSFER_FW : TRANSFER_INJECT;
  for (int l = 0; l <= nCoarse; l++) {
    PrecondLevel& V = M->lev[l];
    snprintf(who, sizeof who, "MG (level %d)", l);
    if (l) precond_level_vectors(V, fn, who, false);
    HostRows h = sgs_download(V.A); // once: the restriction reads the rows whole, the smoother's plan compacts them
    if (l < nCoarse && fw) mg_fw_build(V, coarse[l], *fw, l);
    else if (l < nCoarse) mg_build_restrict(V, coarse[l], h, f2c_host[l], l);
    snprintf(who, sizeof who, "%s: level %d", fn, l);
    V.sgs = sgs_build(V.A, std::move(h), who);
  }
  HIP_CHECK(hipStreamSynchronize(g.stream));
  return s;
}

sb_pcg* sb_pcg_create_mg(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int nCoarse,
    const sb_matrix* const* coarse, const uint32_t* const* f2c_host)
{
  return mg_create("sb_pcg_create_mg", m, halo, b_host, xexact_host, nCoarse, coarse, f2c_host, nullptr);
}

sb_pcg* sb_pcg_create_mg_p(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int nCoarse,
    const sb_matrix* const* coarse, const uint64_t* const* p_ptr, const uint32_t* const* p_col, const double* const* p_val,
    const double* omega)
{
  const MgFwArgs a = { p_ptr, p_col, p_val, omega };
  return mg_create("sb_pcg_create_mg_p", m, halo, b_host, xexact_host, nCoarse, coarse, nullptr, &a);
}

// the polynomial of a level whose A, n and dinv are set: the interval [lmax / ratio, lmax], d and w.  g: the level's row bounds,
// NULL: computed here where lmax <= 0.0 asks for them.  where: "" or "level l: ", as the messages name the matrix
static void cheb_level(PrecondLevel& V, int steps, double lmax, double ratio, const std::vector<double>* g, const char* fn,
    const char* where)
{
  if (!(lmax > 0.0)) lmax = g ? poly_lmax_bound(*g, fn, where) : poly_lmax_bound(poly_rowbound(V.A, V.dinv), fn, where);
  V.cheb.c = poly_coeffs(steps, lmax, ratio);
  if (!(V.cheb.c.c1 > 0.0 && V.cheb.c.c1 < INFINITY))
    SB_FATAL("%s: %slmax = %g, ratio = %g: 1 / theta is not finite and positive", fn, where, lmax, ratio);
  const size_t nb = (size_t)V.n * sizeof(double) + 4096;
  V.cheb.d = (double*)sb_malloc(nb), V.cheb.w = (double*)sb_malloc(nb);
}

// Between two of the cycle's halo exchanges lies no all-reduce, so what keeps a rank from running two exchanges ahead of a
// neighbour (the two staging areas' condition) is the pull itself: a rank pulls from every rank it pushes to.  That holds where
// the ranks it sends to are the ranks it receives from, as a structurally symmetric matrix gives
static void poly_need_mutual_neighbours(const sb_halo* h, const char* fn)
{
  std::vector<int> to(h->destinations), from(h->sources);
  std::sort(to.begin(), to.end()), std::sort(from.begin(), from.end());
  if (to != from)
    SB_FATAL("%s: rank %d sends halo entries to %zu ranks and receives from %zu others: on several ranks the polynomial needs a "
             "matrix whose ranks are each other's neighbours (a structurally symmetric one)", fn, g.rank, to.size(), from.size());
}

// the polynomial alone: a cycle of one level, whose row bounds the handle keeps.  Several ranks: steps, lmax and ratio are
// collective arguments
sb_pcg* sb_pcg_create_poly(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int steps, double lmax,
    double ratio)
{
  const char* fn = "sb_pcg_create_poly";
  if (steps < 1 || steps > SB_POLY_MAX_STEPS) SB_FATAL("%s: steps = %d: the polynomial has 1 to %d steps", fn, steps, SB_POLY_MAX_STEPS);
  if (ratio == 0.0) ratio = 16.0;
  if (!(ratio > 1.0 && ratio < INFINITY)) SB_FATAL("%s: ratio = %g: lmax / lmin must be finite and greater than 1", fn, ratio);
  if (!(lmax < INFINITY)) SB_FATAL("%s: lmax = %g: the caller's lmax must be finite (0.0 or less: the bound)", fn, lmax);
  sb_pcg* s      = precond_create(fn, "Chebyshev polynomial", 4, m, halo, b_host, xexact_host, 0, nullptr, true);
  PrecondPlan* M = s->pre;
  M->smoother = SMOOTH_CHEB, M->steps = M->coarseSteps = steps;
  if (s->halo) { // several ranks: the row bound reads dinv at the halo columns; the cycle exchanges z ahead of its SpMVs
    poly_need_mutual_neighbours(s->halo, fn);
    halo_exchange(s->halo, s->dinv, nullptr);
    HIP_CHECK(hipStreamSynchronize(g.stream));
    M->lev[0].halo = s->halo;
  }
  M->g = poly_rowbound(m, s->dinv);
  if (s->halo && !(lmax > 0.0)) { // the largest bound of any rank's rows: MAX is exact and order-free
    lmax = poly_lmax_bound(M->g, fn, "");
    sb_h2d(g.scalar, &lmax, sizeof lmax);
    sb_comm_reduction(g.scalar, 0);
    sb_d2h(&lmax, g.scalar, sizeof lmax);
  }
  cheb_level(M->lev[0], steps, lmax, ratio, &M->g, fn, "");
  HIP_CHECK(hipStreamSynchronize(g.stream));
  return s;
}

sb_pcg* sb_pcg_create_mg_poly(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int nCoarse,
    const sb_matrix* const* coarse, const uint64_t* const* p_ptr, const uint32_t* const* p_col, const double* const* p_val,
    const double* omega, int steps, int coarse_steps, double lmax, double ratio)
{
  const char* fn = "sb_pcg_create_mg_poly";
  need_init();
  if (steps < 1 || steps > SB_POLY_MAX_STEPS) SB_FATAL("%s: steps = %d: the smoother has 1 to %d steps", fn, steps, SB_POLY_MAX_STEPS);
  if (coarse_steps == 0) coarse_steps = steps;
  if (coarse_steps < 1 || coarse_steps > SB_POLY_MAX_STEPS)
    SB_FATAL("%s: coarse_steps = %d: the coarsest level's polynomial has 1 to %d steps (0: as many as steps)", fn, coarse_steps,
        SB_POLY_MAX_STEPS);
  if (ratio == 0.0) ratio = 4.0;
  if (!(ratio > 1.0 && ratio < INFINITY)) SB_FATAL("%s: ratio = %g: lmax / lmin must be finite and greater than 1", fn, ratio);
  if (!(lmax < INFINITY)) SB_FATAL("%s: lmax = %g: the caller's lmax must be finite (0.0 or less: the bound of every level)", fn, lmax);
  const MgFwArgs a = { p_ptr, p_col, p_val, omega };
  mg_check_hierarchy(fn, m, nCoarse, coarse, nullptr, &a);
  char who[64], where[32];
  snprintf(who, sizeof who, "MG-Chebyshev (level %d)", 0);
  sb_pcg* s      = precond_create(fn, who, 5, m, halo, b_host, xexact_host, nCoarse, coarse);
  PrecondPlan* M = s->pre;
  M->smoother = SMOOTH_CHEB, M->transfer = TRANSFER_FW, M->steps = steps, M->coarseSteps = coarse_steps;
  for (int l = 0; l <= nCoarse; l++) {
    snprintf(who, sizeof who, "MG-Chebyshev (level %d)", l);
    if (l) precond_level_vectors(M->lev[l], fn, who, true);
    snprintf(where, sizeof where, "level %d: ", l);
    cheb_level(M->lev[l], l == nCoarse ? coarse_steps : steps, lmax, ratio, nullptr, fn, where);
    if (l < nCoarse) mg_fw_transfers(M->lev[l], coarse[l], a, l);
  }
  HIP_CHECK(hipStreamSynchronize(g.stream));
  return s;
}

int sb_pcg_precond(const sb_pcg* s) { return s->pre ? s->pre->kind : 0; }

// the levels that can be asked about: none of a diagonal's or a polynomial's, one of the sweeps'
int sb_pcg_levels(const sb_pcg* s) { return !s->pre || s->pre->kind == 4 ? 0 : (int)s->pre->lev.size(); }
static const PrecondLevel& precond_level(const sb_pcg* s, int l, const char* fn)
{
  if (l < 0 || l >= sb_pcg_levels(s)) SB_FATAL("%s: level %d of a handle with %d levels", fn, l, sb_pcg_levels(s));
  return s->pre->lev[l];
}
uint32_t sb_pcg_level_rows(const sb_pcg* s, int l) { return precond_level(s, l, "sb_pcg_level_rows").n; }
// (a Chebyshev-smoothed level has no SgsPlan: no colours)
int sb_pcg_level_colours(const sb_pcg* s, int l)
{
  const SgsPlan* P = precond_level(s, l, "sb_pcg_level_colours").sgs;
  return P ? (int)P->nC : 0;
}

// level 0's sweeps, NULL where the handle has none
static const SgsPlan* precond_sweeps(const sb_pcg* s) { return s->pre ? s->pre->lev[0].sgs : nullptr; }
int sb_pcg_colours(const sb_pcg* s) { return precond_sweeps(s) ? (int)precond_sweeps(s)->nC : 0; }
void sb_pcg_colouring(const sb_pcg* s, uint32_t* colour_host)
{
  need_init();
  const SgsPlan* P = precond_sweeps(s);
  if (!P) SB_FATAL("sb_pcg_colouring: the handle has a diagonal preconditioner (sb_pcg_create_sgs makes the coloured one)");
  const std::vector<uint32_t> o2n = old_to_device_rows(s->A);
  for (uint32_t i = 0; i < s->A->nr; i++) colour_host[i] = P->colour[o2n[i]];
}

int sb_pcg_poly_steps(const sb_pcg* s) { return s->pre ? s->pre->steps : 0; }
static void poly_coeffs_out(const PolyCoef& c, double* out)
{
  out[0] = c.c1;
  for (int j = 2; j <= c.steps; j++) out[2 * j - 3] = c.a[j], out[2 * j - 2] = c.b[j];
}

static const PolyCoef& need_poly(const sb_pcg* s, const char* fn)
{
  if (!s->pre || s->pre->kind != 4) SB_FATAL("%s: the handle has another preconditioner (sb_pcg_create_poly makes the polynomial one)", fn);
  return s->pre->lev[0].cheb.c;
}
void sb_pcg_poly_interval(const sb_pcg* s, double out[2])
{
  const PolyCoef& c = need_poly(s, "sb_pcg_poly_interval");
  out[0] = c.lmin, out[1] = c.lmax;
}
void sb_pcg_poly_coeffs(const sb_pcg* s, double* out) { poly_coeffs_out(need_poly(s, "sb_pcg_poly_coeffs"), out); }
void sb_pcg_poly_rowbound(const sb_pcg* s, double* g_host)
{
  need_init();
  need_poly(s, "sb_pcg_poly_rowbound");
  const std::vector<uint32_t> o2n = old_to_device_rows(s->A);
  for (uint32_t i = 0; i < s->A->nr; i++) g_host[i] = s->pre->g[o2n[i]];
}

static const PolyCoef& need_mgp_level(const sb_pcg* s, int l, const char* fn)
{
  if (!s->pre || s->pre->kind != 5)
    SB_FATAL("%s: the handle has another preconditioner (sb_pcg_create_mg_poly makes the Chebyshev-smoothed cycle)", fn);
  return precond_level(s, l, fn).cheb.c;
}
int sb_pcg_mg_poly_level_steps(const sb_pcg* s, int l) { return need_mgp_level(s, l, "sb_pcg_mg_poly_level_steps").steps; }
void sb_pcg_mg_poly_interval(const sb_pcg* s, int l, double out[2])
{
  const PolyCoef& c = need_mgp_level(s, l, "sb_pcg_mg_poly_interval");
  out[0] = c.lmin, out[1] = c.lmax;
}
void sb_pcg_mg_poly_coeffs(const sb_pcg* s, int l, double* out) { poly_coeffs_out(need_mgp_level(s, l, "sb_pcg_mg_poly_coeffs"), out); }
