// sbhip_cg.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its
// static context): the device-resident CG loop.
// ===========================================================================
// CG
// ===========================================================================
enum { R_WAXPBY = 0, R_SPMVM = 1, R_DDOT = 2, R_COMM = 3 };

// single precision (sbhip_sp.inc.h): the sb_cg_* calls below hand a solver made by sb_cg_create_f32 (prec 1) to these
static void sp_cg_free_arrays(sb_cg* s);
static int sp_launches_per_body(const sb_cg* s);
static bool sp_fusep_plan(sb_cg* s);
static void sp_cg_start(sb_cg* s, int itermax, double eps);
static void sp_cg_run_iters(sb_cg* s, int iters);
static int sp_cg_finish(sb_cg* s);
static int sp_cg_history(const sb_cg* s, double* rr_out, int rr_cap, double* pAp_out, int pAp_cap, int* n_pAp);
static void sp_cg_counters(const sb_cg* s, int out[5]);
static double sp_cg_check_residual(const sb_cg* s);
static const sb_matrix* sp_mirror_selected(const sb_matrix* m);

// events that time kernels inside the loop: created without the system-scope fence a default event carries (SB_EVENT_FLAGS
// overrides the creation flags; 0 = default events)
static unsigned timing_event_flags()
{
  static const unsigned f = getenv("SB_EVENT_FLAGS") ? (unsigned)strtoul(getenv("SB_EVENT_FLAGS"), nullptr, 0) : (unsigned)hipEventDisableSystemFence;
  return f;
}
static void mark(sb_cg* s, int region)
{ // region = the region that ENDS here (-1: start marker)
  if (!s->timing) return;
  if (s->evUsed == s->ev.size()) {
    hipEvent_t e;
    HIP_CHECK(hipEventCreate(&e));
    s->ev.push_back(e);
    s->evRegion.push_back(-1);
  }
  s->evRegion[s->evUsed] = region;
  HIP_CHECK(hipEventRecord(s->ev[s->evUsed], g.stream));
  s->evUsed++;
}

// Per-kernel breakdown of the loop (bench.py): with sb_cg_phase_timing on, an event follows every launch of a loop
// body; the time between two consecutive events belongs to the phase that ENDS at the second one.  Events serialise
// nothing the stream does not already serialise, but each costs ~1 us of its own: the clean it/s is never taken with
// them on.
enum { PH_P_UPDATE = 0, PH_HALO = 1, PH_SPMV = 2, PH_ALPHA = 3, PH_R_UPDATE = 4, PH_BETA = 5, PH_DOT_PASS = 6, PH_COUNT = 7 };
static void phase_mark(sb_cg* s, int ph)
{ // ph = the phase that ends here (-1: start marker)
  if (!s->phaseTiming) return;
  if (s->phUsed == s->phEv.size()) {
    hipEvent_t e;
    HIP_CHECK(hipEventCreateWithFlags(&e, timing_event_flags()));
    s->phEv.push_back(e);
    s->phId.push_back(-1);
  }
  s->phId[s->phUsed] = ph;
  HIP_CHECK(hipEventRecord(s->phEv[s->phUsed], g.stream));
  s->phUsed++;
}

// ---- where the loop's vectors live ------------------------------------------------------------------------------------------
// r, Ap, x, b, p, p' (and xexact) sit in ONE allocation, laid out by vec_layout (sbhip_launch.inc.h).  Which memory that is moves
// the CG step of the section-8d loop by up to 10 %: the upload's placement tuner has measured a good one together with the
// matrix's own placement (sb_matrix::vecArena) and the first sb_cg of a matrix takes it; a second sb_cg on the same matrix while
// the first is alive allocates its own.
static void cg_point_vectors(sb_cg* s, char* slab, bool hasExact)
{
  const VecLayout L = vec_layout(s->nr, s->nc, hasExact, s->vecPad);
  auto at = [&](size_t o) { return reinterpret_cast<double*>(slab + o); };
  s->vecSlab = slab;
  s->r = at(L.r), s->Ap = at(L.Ap), s->x = at(L.x), s->b = at(L.b);
  s->p = at(L.p); // nc = nr + externals (src/CGSolver.c:70)
  s->pbuf[0] = s->p;
  s->pbuf[1] = at(L.p2); // second p of the fused p update (fusep_plan)
  s->xexact  = hasExact ? at(L.xexact) : nullptr;
}

static void apply_dot_order(sb_cg* s);

sb_cg* sb_cg_create(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host)
{
  need_init();
  SB_NEED_PREC(m, 2, "sb_cg_create");
  sb_cg* s = new sb_cg();
  s->A = m, s->halo = halo, s->nr = m->nr, s->nc = m->nc;
  if (halo && halo->nr != m->nr) SB_FATAL("halo plan and matrix disagree on nr");
  if (halo && m->nr + (uint32_t)halo->externalCount != m->nc) SB_FATAL("halo externalCount != nc-nr");
  const size_t nb = (size_t)m->nr * sizeof(double);
  // r, Ap, x, b, p, p' (and xexact) in ONE allocation: the matrix's tuned arena if it is free, else an allocation of their own
  s->vecPad       = getenv("SB_CG_VEC_PAD_KB") ? (size_t)atol(getenv("SB_CG_VEC_PAD_KB")) << 10 : 0;
  s->vecSlabBytes = vec_layout(s->nr, s->nc, xexact_host != nullptr, s->vecPad).total;
  {
    sb_matrix* A = const_cast<sb_matrix*>(m);
    if (A->vecArena && !A->vecArenaBusy && s->vecPad == 0 && s->vecSlabBytes <= A->vecArenaBytes) {
      A->vecArenaBusy = true, s->vecFromArena = true;
      cg_point_vectors(s, A->vecArena, xexact_host != nullptr);
    } else {
      cg_point_vectors(s, (char*)sb_malloc(s->vecSlabBytes), xexact_host != nullptr);
    }
  }
  double* tmp = scratch_ws(0, m->nr);
  sb_h2d(tmp, b_host, nb);
  sb_permute(m, tmp, s->b);
  HIP_CHECK(hipStreamSynchronize(g.stream));
  if (xexact_host) {
    sb_h2d(tmp, xexact_host, nb);
    sb_permute(m, tmp, s->xexact);
    HIP_CHECK(hipStreamSynchronize(g.stream));
  }
  s->S         = (CgScalars*)sb_malloc(sizeof(CgScalars));
  HIP_CHECK(hipMemset(s->S, 0, sizeof(CgScalars))); // never an uninitialised failure flag (sb_cg_start points the push kernels at it)
  s->nPartials = (m->nr + 255) / 256;
  // level-0 partials: 4 per 256 rows; the tail beyond the last chunk stays +0.0
  s->partials = (double*)sb_malloc((4 * (size_t)s->nPartials + 4) * sizeof(double));
  HIP_CHECK(hipMemsetAsync(s->partials, 0, (4 * (size_t)s->nPartials + 4) * sizeof(double), g.stream));
  s->hist_cap  = 0;
  s->rr_hist = s->pAp_hist = nullptr;
  s->partials2 = (double*)sb_malloc((4 * (size_t)s->nPartials + 4) * sizeof(double));
  HIP_CHECK(hipMemsetAsync(s->partials2, 0, (4 * (size_t)s->nPartials + 4) * sizeof(double), g.stream));
  s->fused      = 1;
  s->timing     = false;
  s->evUsed     = 0;
  s->loop_ms    = 0.f;
  s->spmvTiming = false;
  s->spmvEvUsed = 0;
  s->k_next     = 1;
  s->started    = false;
  HIP_CHECK(hipEventCreate(&s->evLoop0));
  HIP_CHECK(hipEventCreate(&s->evLoop1));
  for (double& v : s->region_ms) v = 0.0;
  apply_dot_order(s);
  return s;
}

// (lab: tools/placement_lab2.py) device addresses of the loop's vectors: r, p (both buffers), Ap, x, b, partials
void sb_cg_debug_ptrs(const sb_cg* s, unsigned long long out[8])
{
  const void* v[8] = { s->r, s->pbuf[0], s->pbuf[1], s->Ap, s->x, s->b, s->partials, s->S };
  for (int i = 0; i < 8; i++) out[i] = (unsigned long long)v[i];
}

// The push kernels of a solve also look at ITS failure flag (the control block's; poisoning: kernels.hip.h).  on: sb_cg_start /
// sp_cg_start point the plan at `flag` -- per solve, not at create: the plan is shared, and a second sb_cg on the same halo must
// not redirect a running loop's pushes to a control block that is not in use.  !on: the flag's owner is being freed;
// a plan that still points at it lets go.
static void halo_push_watch(sb_halo* h, const int* flag, bool on)
{
  if (!h || !h->p2p || (h->push.p2pErr == flag) == on) return;
  h->push.p2pErr = on ? flag : nullptr;
  HIP_CHECK(hipStreamSynchronize(g.stream));
  HIP_CHECK(hipMemcpy(h->dPush, &h->push, sizeof h->push, hipMemcpyHostToDevice));
}

void sb_cg_free(sb_cg* s)
{
  if (!s) return;
  HIP_CHECK(hipStreamSynchronize(g.stream));
  halo_push_watch(s->halo, &s->S->p2p_error, false);
  for (hipEvent_t e : s->ev) HIP_CHECK(hipEventDestroy(e));
  for (hipEvent_t e : s->spmvEv) HIP_CHECK(hipEventDestroy(e));
  for (hipEvent_t e : s->phEv) HIP_CHECK(hipEventDestroy(e));
  HIP_CHECK(hipEventDestroy(s->evLoop0));
  HIP_CHECK(hipEventDestroy(s->evLoop1));
  if (s->vecFromArena) const_cast<sb_matrix*>(s->A)->vecArenaBusy = false; // r, Ap, x, b, both p buffers, xexact: back to the matrix
  else sb_free(s->vecSlab);
  sb_free(s->S), sb_free(s->partials), sb_free(s->rr_hist), sb_free(s->pAp_hist), sb_free(s->partials2);
  if (s->prec == 1) sp_cg_free_arrays(s);
  delete s;
}

// The dot order of the loop: tree (0, the fixed order of every fused kernel) or seq (1, the reference's sequential sum,
// dot_seq_k).  seq runs the reference's op list (fused = 0) with each of its dots -- r.r of the prologue and of every body,
// p.Ap -- as dot_seq_k; every fused dot, the fused p update and the folded scalar steps are bypassed because fused is 0.
// The caller's fused level is kept (fusedWant) and runs again when the order returns to tree.  Decided once per solve,
// like the fused-p plan: sb_cg_start latches it, so the pieces of one solve never mix orders; a change in between takes
// effect with the next sb_cg_start.
static bool cg_seq(const sb_cg* s)
{
  if (s->seqLatched >= 0) return s->seqLatched > 0;
  return (s->dotOrderWant >= 0 ? s->dotOrderWant : sb_dot_order()) == 1;
}
static void apply_dot_order(sb_cg* s)
{ // what runs: the caller's level, or the reference's op list under seq
  const int fused = cg_seq(s) ? 0 : s->fusedWant;
  if (s->fused != fused) s->fusepPlan = -1;
  s->fused = fused;
}
void sb_cg_set_dot_order(sb_cg* s, int order)
{
  if (order < -1 || order > 1) SB_FATAL("sb_cg_set_dot_order(%d): expected -1 (process default), 0 (tree) or 1 (seq)", order);
  s->dotOrderWant = order;
  if (s->seqLatched < 0) apply_dot_order(s);
}
int sb_cg_dot_order(const sb_cg* s) { return cg_seq(s) ? 1 : 0; }

void sb_cg_set_fused(sb_cg* s, int fused)
{ // 0: the reference's op list; 1 (default): dots fused into their producers (5 launches per body).  Every non-zero level is 1:
  // levels 2 (the vector phase of a body as one launch) and 3 (the scalar steps taken by workgroup 0 of their consumers) were
  // measured slower and removed (docs/LAB_NOTES.md; the code is in git history, 658dd0b)
  s->fusedWant = fused ? 1 : 0;
  apply_dot_order(s);
}
int sb_cg_vector_phase(sb_cg*) { return 0; } // (the one-launch vector phase: removed with fused level 2)

// ---- the launches of the loop's vector and scalar kernels: the loop and the blocking test entries (below) share them ---------
// workgroups of the two vector kernels: 1024 threads (512 workgroups to dispatch instead of 2048: +0.7 % it/s at 128^3,
// measured back to back; SB_VEC_BLOCK=256|512 for comparison)
static uint32_t cg_vec_block()
{
  static const uint32_t vb = getenv("SB_VEC_BLOCK") && atoi(getenv("SB_VEC_BLOCK")) >= 64 ? (uint32_t)atoi(getenv("SB_VEC_BLOCK")) & ~63u : 1024u;
  return vb;
}
static uint32_t cg_vec_cap() { return (uint32_t)g.prop.multiProcessorCount * (2048u / cg_vec_block()); }
// grid of cg_update_p (and cg_update_p_push) over n rows: a thread per two double2, strip-mined past the cap
static uint32_t cg_update_p_grid(uint32_t n)
{
  const uint32_t vb = cg_vec_block();
  return std::max(1u, std::min(cg_vec_cap(), (n / 2 + 1 + vb - 1) / vb));
}
// grid of cg_update_r_k<mode> over n rows: a wave per 256-row group; mode 1 (every workgroup reads all m level-1 values) runs
// one workgroup per CU where the others run two
static uint32_t cg_update_r_grid(uint32_t n, int mode)
{
  const uint32_t vb   = cg_vec_block();
  const uint32_t grid = std::max(1u, std::min(cg_vec_cap(), (((n + 255u) >> 8) + vb / 64 - 1) / (vb / 64)));
  if (mode != 1) return grid;
  // one workgroup per CU (the separate r update runs two): every workgroup reads all m values, so half the workgroups is half
  // that traffic -- 128^3, same box, alternating: 41.6 / 42.1 us per iteration against 42.4 / 42.7 with two (and 43.8 / 44.2
  // with the separate alpha launch)
  static const uint32_t perCu = getenv("SB_ALPHA_WG_PER_CU") ? (uint32_t)std::max(1, atoi(getenv("SB_ALPHA_WG_PER_CU"))) : 1u;
  return std::max(1u, std::min((uint32_t)g.prop.multiProcessorCount * perCu, grid));
}
// cg_update_p<mode>: mode 0 p = r + beta p (which != 0: r + 0.0 r) with the owed x update; 1 / 2 with the beta step at its head,
// from the m level-1 values l1 / from S->local
static void launch_cg_update_p(int mode, uint32_t n, const double* r, double* p, double* x, CgScalars* S, int which, uint32_t m,
    const double* l1, double* rr_hist)
{
  const dim3 grid(cg_update_p_grid(n)), block(cg_vec_block());
  if (mode == 2) hipLaunchKernelGGL(cg_update_p<2>, grid, block, 0, g.stream, n, r, p, x, S, which, m, l1, rr_hist);
  else if (mode == 1) hipLaunchKernelGGL(cg_update_p<1>, grid, block, 0, g.stream, n, r, p, x, S, which, m, l1, rr_hist);
  else if (n) hipLaunchKernelGGL(cg_update_p<0>, grid, block, 0, g.stream, n, r, p, x, S, which, 0u, (const double*)nullptr, (double*)nullptr);
  HIP_CHECK(hipGetLastError());
}
// cg_update_r_k<mode>: mode 0 r -= alpha Ap with the level-1 values of r.r into l1out; 1 / 2 with the alpha step at its head,
// from the m level-1 values l1in / from S->local
static void launch_cg_update_r(int mode, uint32_t n, const double* Ap, double* r, CgScalars* S, double* l1out, const int* stop, uint32_t m,
    const double* l1in, double* rr_hist, double* pAp_hist)
{
  const dim3 grid(cg_update_r_grid(n, mode)), block(cg_vec_block());
  if (mode == 2) hipLaunchKernelGGL(cg_update_r_k<2>, grid, block, 0, g.stream, n, Ap, r, S, l1out, stop, m, l1in, rr_hist, pAp_hist);
  else if (mode == 1) hipLaunchKernelGGL(cg_update_r_k<1>, grid, block, 0, g.stream, n, Ap, r, S, l1out, stop, m, l1in, rr_hist, pAp_hist);
  else
    hipLaunchKernelGGL(cg_update_r_k<0>, grid, block, 0, g.stream, n, Ap, r, S, l1out, stop, 0u, (const double*)nullptr, (double*)nullptr,
        (double*)nullptr);
  HIP_CHECK(hipGetLastError());
}
// the x update the last body left owing, over n rows (p0 / p1: the buffers of the even / odd bodies)
static void launch_cg_x_finalize(uint32_t n, double* x, const double* p0, const double* p1, const CgScalars* S)
{
  if (n == 0) return;
  hipLaunchKernelGGL(cg_x_finalize, dim3(stream_grid(n, 256)), dim3(256), 0, g.stream, n, x, p0, p1, S);
  HIP_CHECK(hipGetLastError());
}
// w = x + (*beta_dev) y of the reference-shaped op list (256-thread workgroups)
static void launch_waxpby_sdev(uint32_t n, const double* x, const double* beta_dev, const double* y, double* w, const int* stop)
{
  if (n == 0) return;
  hipLaunchKernelGGL(waxpby_sdev_k, dim3(stream_grid(n / 2 + 1, 256)), dim3(256), 0, g.stream, n, x, beta_dev, y, w, stop);
  HIP_CHECK(hipGetLastError());
}
// cg_scalar_k<mode, reduce>: one workgroup
static void launch_cg_scalar(int mode, bool reduce, uint32_t m, const double* q, CgScalars* S, double* rr_hist, double* pAp_hist, int to_local,
    int defer_x, int l1)
{
  const dim3 grid(1), block(1024);
#define SB_CG_SCALAR(MODE)                                                                                                          \
  {                                                                                                                                \
    if (reduce) hipLaunchKernelGGL((cg_scalar_k<MODE, true>), grid, block, 0, g.stream, m, q, S, rr_hist, pAp_hist, to_local, defer_x, l1); \
    else hipLaunchKernelGGL((cg_scalar_k<MODE, false>), grid, block, 0, g.stream, m, q, S, rr_hist, pAp_hist, to_local, defer_x, l1);       \
  }
  if (mode == 0) SB_CG_SCALAR(0)
  else if (mode == 1) SB_CG_SCALAR(1)
  else if (mode == 2) SB_CG_SCALAR(2)
  else SB_FATAL("launch_cg_scalar: unknown mode %d", mode);
#undef SB_CG_SCALAR
  HIP_CHECK(hipGetLastError());
}

template <int MODE> static void scalar_launch(sb_cg* s, int defer_x, const double* q, int l1 = 0);
static int pAp_is_level1(const sb_cg* s);
static int fusealpha_plan(sb_cg* s, int l1, uint32_t vb);
static int fusebeta_plan(sb_cg* s, uint32_t vb);

static bool spmv_can_fuse_dot(const sb_cg* s);
// The p update inside the SpMV (pack.hip.h: spmv_prog_fusep; 4 launches per body: SpMV | alpha | r update | beta): where the
// matrix allows it (spmv_fusep_possible), in the default loop (fused = 1), on one rank or with the halo over peer-mapped
// memory (the push kernel then forms the boundary values itself; a send / recv exchange needs p in memory first).
// SB_FUSE_P=0 keeps the separate p update.
static bool fusep_plan(sb_cg* s)
{
  // Inside a solve the answer is the one sb_cg_start latched: the fused path keeps p double-buffered and picks the
  // buffer from the body count, the in-place path does not -- a body of the other kind in the middle of a solve (the matrix's
  // kernel mode or the wish changed between two sb_cg_run_iters pieces) would read the wrong p.  Such a change takes effect with
  // the next sb_cg_start.
  if (s->started && s->fusepLatched >= 0) return s->fusepLatched > 0;
  if (s->fusepPlan < 0) { // (the wish is decided once; whether it applies follows the matrix's kernel mode and the data plane)
    const char* env = getenv("SB_FUSE_P");
    s->fusepPlan    = (s->fusepWant >= 0 ? s->fusepWant != 0 : env ? atoi(env) != 0 : SB_FUSE_P_DEFAULT) ? 1 : 0;
  }
  bool ok = s->fusepPlan > 0 && s->fused == 1 && s->nr > 0 && spmv_fusep_possible(s->A);
  if (ok && multi_rank()) ok = s->halo ? halo_p2p_active(s->halo) : true;
  return ok;
}
// The halo exchange folded into the streaming loop's own kernels (sb_comm_halo_fold; kernels.hip.h: cg_update_p_push |
// spmv_scs64_halo | alpha | r update | beta -- 5 launches, both precisions).  Taken when ALL hold, today's body otherwise:
// the switch is on; several ranks with a halo plan whose peer-mapped path is active; the fused loop under the tree order;
// Sell-C-sigma with C = 64 and the reference-layout kernel selected (spmv_scs64 / spmv_scs64_f32: not the row programs, not
// the SP mirror).  CRS, generic C, the mirror kernels, seq, fused = 0 and the communicator's plane keep their bodies.
// Inside a solve the answer is the one sb_cg_start / sp_cg_start latched, like the fused-p plan and the dot order: the two
// bodies use the staging area differently (the folded one never fills the tail of p), so the pieces of one solve must not
// mix them; a change of the switch takes effect with the next start.
static bool halo_fold_plan(sb_cg* s)
{
  if (s->started && s->foldLatched >= 0) return s->foldLatched > 0;
  if (!sb_comm_halo_fold_selected()) return false;
  const sb_matrix* A = s->A;
  if (!multi_rank() || !s->halo || !halo_p2p_active(s->halo) || !p2p_dots() || s->fused != 1 || cg_seq(s) || s->nr == 0) return false;
  if (A->fmt != 1 || A->C != 64) return false;
  return s->prec == 1 ? sp_mirror_selected(A) == nullptr : !spmv_uses_patterns(A);
}
int sb_cg_halo_fold(sb_cg* s)
{
  if (s->seqLatched < 0) apply_dot_order(s);
  return halo_fold_plan(s) ? 1 : 0;
}

// kernel launches per loop body.  One rank: 5 (p update | SpMV | alpha | r update | beta); 0 = the reference's op list.
// Several ranks add the halo kernels (peer-mapped: the push, 0 with the push inside the SpMV launch, + a pull where the
// SpMV is not the pattern kernel; otherwise the pack kernel in front of the send / recv group) and, without the in-kernel
// all-reduce, one more kernel per dot (local reduce | all-reduce | scalar step) -- the all-reduce / send-recv calls
// themselves are counted by sb_cg_collectives_per_body.  With the exchange folded into the streaming loop's own kernels
// (halo_fold_plan above): 5, both precisions.
int sb_cg_launches_per_body(sb_cg* s)
{
  if (s->seqLatched < 0) apply_dot_order(s); // (the process default may have changed since the last call)
  if (halo_fold_plan(s)) return 5; // p update + push | SpMV + pull | alpha | r update | beta (both precisions)
  if (s->prec == 1) return sp_launches_per_body(s);
  int base = fusep_plan(s) ? 4 : s->fused ? 5 : 0;
  if (base >= 4 && fusealpha_plan(s, fusep_plan(s) ? 1 : pAp_is_level1(s), 1024u)) base -= 1; // (alpha step inside the r update)
  if (base >= 4 && fusebeta_plan(s, 1024u)) base -= 1;                                          // (beta step inside the p update)
  if (!multi_rank() || base == 0) return base;
  int n = base;
  if (s->halo) {
    const bool inSpmv = halo_p2p_active(s->halo) && spmv_can_fuse_dot(s) && spmv_uses_patterns(s->A);
    if (inSpmv) n += (s->halo->totalSend && !g.pushInside) ? 1 : 0;
    else if (halo_p2p_active(s->halo)) n += (s->halo->totalSend ? 1 : 0) + (s->halo->indegree ? 1 : 0);
    else n += s->halo->totalSend ? 1 : 0;
  }
  if (!p2p_dots()) n += 2;
  return n;
}
// communicator calls per loop body (RCCL / transport): 2 all-reduces + 1 send-recv group without the peer-mapped paths
int sb_cg_collectives_per_body(sb_cg* s)
{
  if (s->seqLatched < 0) apply_dot_order(s);
  if (!multi_rank() || !s->fused) return 0;
  return (p2p_dots() ? 0 : 2) + (s->halo && !halo_p2p_active(s->halo) ? 1 : 0);
}

// 1 / 0: take / do not take the p update inside the SpMV where the matrix and the data plane allow it; -1: the default
// (SB_FUSE_P, else the library's).  sb_cg_fuse_p: what the loop will do.
void sb_cg_set_fuse_p(sb_cg* s, int on)
{
  s->fusepWant = on < 0 ? -1 : on != 0;
  s->fusepPlan = -1;
}
int sb_cg_fuse_p(sb_cg* s)
{
  if (s->seqLatched < 0) apply_dot_order(s);
  return (s->prec == 1 ? sp_fusep_plan(s) : fusep_plan(s)) ? 1 : 0;
}

// hipGraph replay of a loop body was measured slower (-7 % at 128^3, -13 ... -35 % at 64^3: docs/LAB_NOTES.md) and removed;
// the call stays for callers that still pass SB_GRAPH / --graph
void sb_cg_set_graph(sb_cg*, int) {}

void sb_cg_spmv_timing(sb_cg* s, int on)
{
  s->spmvTiming = on != 0;
  s->spmvEvUsed = 0;
}

double sb_cg_spmv_ms(sb_cg* s, int* launches)
{ // sum of the event-bracketed SpMV launches since sb_cg_spmv_timing(s, 1)
  HIP_CHECK(hipStreamSynchronize(g.stream));
  double total = 0.0;
  int n        = 0;
  for (size_t i = 0; i + 1 < s->spmvEvUsed; i += 2) {
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, s->spmvEv[i], s->spmvEv[i + 1]));
    total += ms;
    n++;
  }
  if (launches) *launches = n;
  return total;
}

// lab call (tools/placement_lab11.py): the event-bracketed SpMV launches since sb_cg_spmv_timing(s, 1), one by one (us); returns
// how many there are (at most `cap` are written)
int sb_cg_spmv_us_series(sb_cg* s, float* out, int cap)
{
  HIP_CHECK(hipStreamSynchronize(g.stream));
  int n = 0;
  for (size_t i = 0; i + 1 < s->spmvEvUsed; i += 2, n++) {
    if (n >= cap) continue;
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, s->spmvEv[i], s->spmvEv[i + 1]));
    out[n] = 1e3f * ms;
  }
  return n;
}

void sb_cg_phase_timing(sb_cg* s, int on)
{
  s->phaseTiming = on != 0;
  s->phUsed      = 0;
}

int sb_cg_phase_ms(sb_cg* s, double ms_out[8], int count_out[8])
{ // summed duration and number of occurrences of every phase since sb_cg_phase_timing(s, 1); returns the number of phases
  HIP_CHECK(hipStreamSynchronize(g.stream));
  for (int i = 0; i < 8; i++) ms_out[i] = 0.0, count_out[i] = 0;
  for (size_t i = 1; i < s->phUsed; i++) {
    const int ph = s->phId[i];
    if (ph < 0) continue; // a start marker: the time in front of it (host gaps between run_iters calls) belongs to nobody
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, s->phEv[i - 1], s->phEv[i]));
    ms_out[ph] += ms, count_out[ph]++;
  }
  return PH_COUNT;
}

void sb_cg_counters(const sb_cg* s, int out[5])
{ // stop, stop_next, iters, n_rr, n_pAp of the device control block
  if (s->prec == 1) return sp_cg_counters(s, out);
  HIP_CHECK(hipStreamSynchronize(g.stream));
  CgScalars h;
  HIP_CHECK(hipMemcpy(&h, s->S, sizeof h, hipMemcpyDeviceToHost));
  out[0] = h.stop, out[1] = h.stop_next, out[2] = h.iters, out[3] = h.n_rr, out[4] = h.n_pAp;
}

static bool spmv_can_fuse_dot(const sb_cg* s)
{ // p.Ap partials in the SpMV epilogue: the wave-per-chunk kernels (SCS C=64, or CRS through its mirror)
  return s->fused && (s->A->fmt == 1 ? s->A->C == 64 : spmv_uses_patterns(s->A));
}

// levels 1-2 of the reduction + the scalar step: one 1-workgroup launch after the producer
// (several ranks: local sum -> RCCL all-reduce in place on the stream -> scalar step;
// MPI_Allreduce of src/comm.c:659)
// l1: q holds level-1 values (cg_update_r_k) instead of level-0 partials
template <int MODE> static void scalar_launch(sb_cg* s, int defer_x, const double* q, int l1)
{
  if (!q) q = s->partials;
  uint32_t m = s->nPartials;
  if (s->seqLatched > 0) m = 1, l1 = 1; // (seq: the rank's whole sum is q[0], cg_dot)
  if (multi_rank() && p2p_dots()) { // local reduce, in-kernel all-reduce and scalar step in ONE launch
    hipLaunchKernelGGL((cg_scalar_p2p_k<MODE>), dim3(1), dim3(1024), 0, g.stream, m, q,
        s->S, s->rr_hist, s->pAp_hist, defer_x, (const P2PView*)g.p2pView, ++g.p2pSeq, l1,
        (const int*)(s->halo && s->halo->p2p ? s->halo->err : nullptr));
    HIP_CHECK(hipGetLastError());
    return;
  }
  launch_cg_scalar(MODE, true, m, q, s->S, s->rr_hist, s->pAp_hist, multi_rank() ? 1 : 0, defer_x, l1);
  if (multi_rank()) {
    mark(s, R_DDOT);
    sb_comm_reduction(&s->S->local, 1);
    mark(s, R_COMM);
    launch_cg_scalar(MODE, false, s->nPartials, q, s->S, s->rr_hist, s->pAp_hist, 0, defer_x, 0);
  }
}

// 1: LEVEL-1 values of p.Ap (one per 256 rows) -- from the SpMV's fused dot, or (fused loop behind a kernel without a dot of
// its own) from the dot pass dot_l1_k; 0: level-0 partials (the reference's op list)
static int pAp_is_level1(const sb_cg* s) { return spmv_can_fuse_dot(s) || (s->fused && s->nr) ? 1 : 0; }

// The scalar steps inside their consumers' launches (kernels.hip.h: cg_update_r_k<ALPHA>, cg_update_p<BETA>): EVERY workgroup of
// the consumer takes the step itself -- nobody waits for anybody --, workgroup 0 records it.  Returns the mode: 0 the separate
// scalar launch; 1 (one rank) each workgroup reduces the producer's level-1 values itself; 2 (several ranks on the
// communicator's collectives) the sum is already reduced and all-reduced into S->local by the two launches before, the third
// launch of that dot goes.  The peer-mapped plane keeps its one-launch step (local reduce, exchange and step: cg_scalar_p2p_k).
// Needs level-1 values from the producer and 1024-thread workgroups.  SB_FUSE_ALPHA=0 / sb_cg_set_fuse_alpha(s, 0) and
// SB_FUSE_BETA=0 / sb_cg_set_fuse_beta(s, 0): the separate launches.
static int fold_mode(sb_cg* s, int l1, uint32_t vb)
{
  if (!s->fused || !l1 || vb != 1024u) return 0;
  if (multi_rank()) return p2p_dots() ? 0 : 2;
  return 1;
}
static int fusealpha_plan(sb_cg* s, int l1, uint32_t vb)
{
  static const int env = getenv("SB_FUSE_ALPHA") ? atoi(getenv("SB_FUSE_ALPHA")) != 0 : -1;
  const bool want = s->fuseAlphaWant >= 0 ? s->fuseAlphaWant != 0 : env >= 0 ? env != 0 : true;
  return want ? fold_mode(s, l1, vb) : 0;
}
// (the beta step rides in the p update's launch: only where the p update is a launch of its own, i.e. not inside the SpMV)
static int fusebeta_plan(sb_cg* s, uint32_t vb)
{
  static const int env = getenv("SB_FUSE_BETA") ? atoi(getenv("SB_FUSE_BETA")) != 0 : -1;
  const bool want = s->fuseBetaWant >= 0 ? s->fuseBetaWant != 0 : env >= 0 ? env != 0 : true;
  if (!want || fusep_plan(s)) return 0;
  return fold_mode(s, 1, vb);
}
void sb_cg_set_fuse_alpha(sb_cg* s, int on) { s->fuseAlphaWant = on < 0 ? -1 : on != 0; }
void sb_cg_set_fuse_beta(sb_cg* s, int on) { s->fuseBetaWant = on < 0 ? -1 : on != 0; }

// several ranks, communicator's collectives: local levels 1-2 of a dot into S->local, all-reduced in place on the stream
// (MPI_Allreduce of src/comm.c:659); the step itself is taken by the consumer (fold mode 2) or by cg_scalar_k<MODE, false>
template <int MODE> static void scalar_reduce_only(sb_cg* s, const double* q, int l1)
{
  launch_cg_scalar(MODE, true, s->nPartials, q, s->S, s->rr_hist, s->pAp_hist, 1, 0, l1);
  mark(s, R_DDOT);
  sb_comm_reduction(&s->S->local, 1);
  mark(s, R_COMM);
}

// alpha step (src/CGSolver.c:124-126) and r -= alpha Ap + the r.r values of the next body (:128, :112): two launches, or one
static void alpha_and_r_update(sb_cg* s, int l1, const int* stop)
{
  const uint32_t n = s->nr;
  const int mode = fusealpha_plan(s, l1, cg_vec_block());
  if (mode) {
    if (mode == 2) {
      scalar_reduce_only<2>(s, s->partials, l1);
      phase_mark(s, PH_ALPHA);
    }
    launch_cg_update_r(mode, n, s->Ap, s->r, s->S, s->partials2, stop, s->nPartials, s->partials, s->rr_hist, s->pAp_hist);
    mark(s, R_WAXPBY);
    phase_mark(s, PH_R_UPDATE);
    return;
  }
  scalar_launch<2>(s, 0, nullptr, l1);
  mark(s, R_DDOT);
  phase_mark(s, PH_ALPHA);
  launch_cg_update_r(0, n, s->Ap, s->r, s->S, s->partials2, stop, 0u, nullptr, nullptr, nullptr);
  mark(s, R_WAXPBY);
  phase_mark(s, PH_R_UPDATE);
}

// beta step / loop test behind the r update (:107, :111-113, :116): its own launch(es), or left owing to the next body's p
// update (cg_update_p<BETA>; flush_beta_fold takes it where no body follows)
static void beta_step_or_owe(sb_cg* s, uint32_t vb)
{
  const int mode = fusebeta_plan(s, vb);
  if (mode) {
    if (mode == 2) scalar_reduce_only<1>(s, s->partials2, 1);
    s->betaFold = mode;
    return;
  }
  scalar_launch<1>(s, 1, s->partials2, 1);
  mark(s, R_DDOT);
  phase_mark(s, PH_BETA);
}
static void flush_beta_fold(sb_cg* s)
{
  if (!s->betaFold) return;
  if (s->betaFold == 2) { // r.r is in S->local already
    launch_cg_scalar(1, false, s->nPartials, s->partials2, s->S, s->rr_hist, s->pAp_hist, 0, 1, 0);
  } else scalar_launch<1>(s, 1, s->partials2, 1);
  mark(s, R_DDOT);
  phase_mark(s, PH_BETA);
  s->betaFold = 0;
}

static void spmv_event(sb_cg* s)
{
  if (!s->spmvTiming) return;
  if (s->spmvEvUsed == s->spmvEv.size()) {
    hipEvent_t e;
    HIP_CHECK(hipEventCreateWithFlags(&e, timing_event_flags()));
    s->spmvEv.push_back(e);
  }
  HIP_CHECK(hipEventRecord(s->spmvEv[s->spmvEvUsed++], g.stream));
}

// The SpMV launch that follows is the one to time: bracket it with two events recorded on the stream.  The events are created
// with hipEventDisableSystemFence (a default event performs a system-scope fence -- L2 write-back and invalidate -- when it is
// recorded, which costs time of its own and slows the work behind it; the HIP headers recommend the flag for timing).
// Measured on one box, same run (tools/ext_timing_check.sh; rocprofv3 of the same loop: 129.8 / 30.7 us on another box):
//   reference-layout SpMV / fused SpMV:  record, no fence 135.7 / 29.3 us;  record, default events 137.7 / 31.3 us;
//   hipExtLaunchKernelGGL's start / stop stamps of the launch itself (SB_SPMV_TIMING=ext) 138.9 / 27.6 and 139.5 / 30.2 us.
// None of them reaches rocprofv3's own begin -> end of the dispatch for the long kernel (it reports 129.8 us for the launches
// of the clean passes, the events pass and the phases pass alike: the kernel is not disturbed, the brackets are wider).
static bool spmv_time_begin(sb_cg* s)
{
  if (!s->spmvTiming) return false;
  static const bool record = !(getenv("SB_SPMV_TIMING") && strcmp(getenv("SB_SPMV_TIMING"), "ext") == 0);
  if (record) {
    spmv_event(s);
    return true;
  }
  while (s->spmvEv.size() < s->spmvEvUsed + 2) {
    hipEvent_t e;
    HIP_CHECK(hipEventCreateWithFlags(&e, timing_event_flags()));
    s->spmvEv.push_back(e);
  }
  g_spmvEvA = s->spmvEv[s->spmvEvUsed], g_spmvEvB = s->spmvEv[s->spmvEvUsed + 1];
  s->spmvEvUsed += 2;
  return true;
}
static void spmv_time_end(sb_cg* s)
{
  if (!s->spmvTiming) return;
  if (g_spmvEvA) g_spmvEvA = g_spmvEvB = nullptr;
  else spmv_event(s);
}

// a dot of the reference's op list into `partials`: the tree order's level-0 partials, or (seq) the rank's sequential sum over
// its nr rows in original row order as the one value the scalar step reads (scalar_launch)
static void cg_dot(sb_cg* s, const double* a, const double* b, const int* stop)
{
  if (s->seqLatched > 0) launch_dot_seq(s->nr, a, b, s->A->permuted ? s->A->oldToNew : nullptr, s->partials, stop);
  else launch_dot_spans(0, s->nr, a, b, nullptr, nullptr, s->S, s->partials, stop);
}

// Ap = A p and the level-0 partials of p.Ap (src/CGSolver.c:123-125): fused into the SpMV epilogue
// where the kernel is wave-per-chunk, otherwise SpMV then a dot pass
static void spmv_and_pAp(sb_cg* s, const int* stop)
{
  const uint32_t n = s->nr;
  if (spmv_can_fuse_dot(s)) {
    spmv_time_begin(s);
    launch_spmv(s->A, s->p, s->Ap, s->partials, stop);
    spmv_time_end(s);
    mark(s, R_SPMVM);
    phase_mark(s, PH_SPMV);
  } else {
    spmv_time_begin(s);
    launch_spmv(s->A, s->p, s->Ap, nullptr, stop);
    spmv_time_end(s);
    mark(s, R_SPMVM);
    phase_mark(s, PH_SPMV);
    if (s->fused && n) { // level-1 values straight away (pAp_is_level1): a quarter of the bytes for the step, which can then ride in the r update
      hipLaunchKernelGGL(dot_l1_k, dim3(vec_stream_grid(n)), dim3(1024), 0, g.stream, n, (const double*)s->p, (const double*)s->Ap,
          s->partials, stop);
      HIP_CHECK(hipGetLastError());
    } else cg_dot(s, s->p, s->Ap, stop);
    phase_mark(s, PH_DOT_PASS);
  }
}

// one loop body of solveCG (src/CGSolver.c:108-128).  Fused path: the r.r partials of the
// NEXT body come out of this body's x/r update, and its beta + loop test are taken right
// after it, so a body is: p update | SpMV (+p.Ap partials) | alpha | x/r update (+r.r
// partials) | beta, loop test.
static void loop_body(sb_cg* s, int k)
{
  const uint32_t n = s->nr;
  const int* stop  = &s->S->stop;
  const uint32_t vb = cg_vec_block(); // (the two vector kernels' workgroups and grids: cg_vec_block, cg_update_p_grid, cg_update_r_grid)
  if (fusep_plan(s)) {
    // p = r + beta p (:114; k = 1: p = r, :109), the owed x update (:127), the halo exchange (:122) and Ap = A p with its p.Ap
    // values (:123-125) in ONE launch (+ the halo push on several ranks): body k reads p_{k-1} in pbuf[(k - 1) & 1] and writes
    // p_k into pbuf[k & 1]
    const int which    = k == 1;
    const double* pold = which ? s->r : s->pbuf[(k - 1) & 1];
    double* pnew       = s->pbuf[k & 1];
    HaloWait hw;
    memset(&hw, 0, sizeof hw);
    const bool halo = multi_rank() && s->halo;
    if (halo) {
      sb_halo* h = s->halo;
      const unsigned long long seq = ++h->seq;
      if (g.pushInside) hw.push = h->dPush, hw.nPush = h->totalSend ? 16u : 0u;
      else if (h->totalSend) {
        hipLaunchKernelGGL(halo_push_fusep_k, dim3(stream_grid(h->totalSend, 256)), dim3(256), 0, g.stream, h->push, pold, s->r,
            (const CgScalars*)s->S, which, seq);
        HIP_CHECK(hipGetLastError());
      }
      phase_mark(s, PH_HALO);
      hw.flags = h->stage + 2 * (size_t)h->externalCount;
      hw.ext   = reinterpret_cast<const double*>(h->stage + (seq & 1ull) * (size_t)h->externalCount);
      hw.src = h->dSrcRank, hw.nsrc = h->indegree, hw.seq = seq, hw.err = h->err;
      hw.stopw = &s->S->stop, hw.timeoutTicks = h->push.timeoutTicks;
    }
    spmv_time_begin(s);
    launch_spmv_fusep(s->A, pold, s->r, pnew, s->x, s->Ap, s->S, which, s->partials, halo ? &hw : nullptr);
    spmv_time_end(s);
    phase_mark(s, PH_SPMV);
    s->p = pnew; // (host-side view: the newest p; cg_x_finalize picks the buffer of the last body that RAN from the device counters)
    alpha_and_r_update(s, 1, stop);
    scalar_launch<1>(s, 1, s->partials2, 1);
    phase_mark(s, PH_BETA);
    return;
  }
  if (halo_fold_plan(s)) {
    // p = r + beta p (:114; k = 1: p = r + 0.0 r, :109) with the owed x update (:127) AND the push of the boundary rows
    // (:122, send side) | Ap = A p with its p.Ap values (:123-125), the halo blocks waiting for the neighbours themselves
    // (:122, receive side) | alpha | r update | beta
    sb_halo* h       = s->halo;
    const int which  = k == 1;
    const dim3 gridV(cg_update_p_grid(n)), blockV(vb);
    const HaloFold& hf = halo_fold_send_plan(h, 0, gridV.x, vb);
    const unsigned long long seq = ++h->seq;
    hipLaunchKernelGGL(cg_update_p_push, gridV, blockV, 0, g.stream, h->push, hf, seq, n, (const double*)s->r, s->p,
        which ? (double*)nullptr : s->x, s->S, which);
    HIP_CHECK(hipGetLastError());
    mark(s, R_WAXPBY);
    phase_mark(s, PH_P_UPDATE);
    uint32_t perI = 0, gridS = 0;
    const ScsHalo hh = halo_fold_spmv_arg(h, s->A, seq, &s->S->stop, &perI, &gridS);
    spmv_time_begin(s);
    launch_spmv_scs64_halo(s->A, s->p, s->Ap, s->partials, stop, hh, perI, gridS);
    spmv_time_end(s);
    mark(s, R_SPMVM);
    phase_mark(s, PH_SPMV);
    alpha_and_r_update(s, 1, stop);
    beta_step_or_owe(s, vb);
    return;
  }
  if (k == 1) {
    launch_cg_update_p(0, n, s->r, s->p, nullptr, s->S, 1, 0u, nullptr, nullptr); // p = r (:109)
    mark(s, R_WAXPBY);
    phase_mark(s, PH_P_UPDATE);
  } else {
    if (!s->fused) { // rtrans = r.r ; beta (:111-113)
      cg_dot(s, s->r, s->r, stop);
      phase_mark(s, PH_DOT_PASS);
      scalar_launch<1>(s, 0, nullptr);
      mark(s, R_DDOT);
      phase_mark(s, PH_BETA);
    }
    // p = r + beta p (:114); fused path: also the x update owed by the previous body (:127) -- and, where the previous body left
    // its beta step / loop test owing, that step at the head of this launch
    if (s->betaFold) launch_cg_update_p(s->betaFold, n, s->r, s->p, s->x, s->S, 0, s->nPartials, s->partials2, s->rr_hist);
    else launch_cg_update_p(0, n, s->r, s->p, s->fused ? s->x : nullptr, s->S, 0, 0u, nullptr, nullptr);
    s->betaFold = 0;
    mark(s, R_WAXPBY);
    phase_mark(s, PH_P_UPDATE);
  }
  HIP_CHECK(hipGetLastError());
  // (the exchange on a second stream behind the interior tiles was measured no faster -- one cross-stream dependency costs
  // ~12 us here, about what it hides -- and removed: docs/LAB_NOTES.md)
  if (multi_rank() && halo_p2p_active(s->halo) && spmv_can_fuse_dot(s) && spmv_uses_patterns(s->A)) {
    // :122-126 over peer-mapped memory with the pull inside the SpMV: the halo-touching tiles (stored
    // last) wait for the neighbours' pushes themselves and read the staging area; interior tiles hide it
    // SB_HALO_PUSH_INSIDE=1: the push rides in the SpMV launch too (its first 16 workgroups) instead of a launch of its
    // own.  Bit-identical (tests/test_gpu_multirank.py runs both); NOT the default: the only place it can be timed here
    // is N ranks sharing one GPU, where it is slower (2 x 128^3: 291 vs 178 us per step -- a rank's waiting tiles keep
    // the other rank's SpMV, and with it its push, off the CUs), and on ranks with a GPU each, where it should save the
    // ~4.5 us launch, it cannot be measured from this box.
    sb_halo* h = s->halo;
    const bool pushInside = g.pushInside;
    HaloWait hw;
    memset(&hw, 0, sizeof hw);
    if (pushInside) {
      ++h->seq;
      hw.push = h->dPush, hw.nPush = h->totalSend ? 16u : 0u;
    } else halo_exchange(h, s->p, stop, nullptr, true, true);
    mark(s, R_COMM);
    phase_mark(s, PH_HALO);
    hw.flags = h->stage + 2 * (size_t)h->externalCount;
    hw.ext   = reinterpret_cast<const double*>(h->stage + (h->seq & 1ull) * (size_t)h->externalCount);
    hw.src = h->dSrcRank, hw.nsrc = h->indegree, hw.seq = h->seq, hw.err = h->err;
    hw.stopw = &s->S->stop, hw.timeoutTicks = h->push.timeoutTicks;
    spmv_time_begin(s);
    launch_spmv(s->A, s->p, s->Ap, s->partials, stop, &hw);
    spmv_time_end(s);
    mark(s, R_SPMVM);
    phase_mark(s, PH_SPMV);
  } else {
    halo_exchange(s->halo, s->p, stop, nullptr, true); // :122
    mark(s, R_COMM);
    if (multi_rank() && s->halo) phase_mark(s, PH_HALO);
    spmv_and_pAp(s, stop);
  }
  if (s->fused) { // alpha; r -= alpha Ap (:128) + next r.r, beta, loop test; x += alpha p (:127) is owed
    // (level-1 values of r.r into partials2: `partials` keeps the layout the p.Ap producers write)
    alpha_and_r_update(s, pAp_is_level1(s), stop);
    beta_step_or_owe(s, vb);
    return;
  }
  scalar_launch<2>(s, 0, nullptr, pAp_is_level1(s));
  mark(s, R_DDOT);
  phase_mark(s, PH_ALPHA);
  if (n) { // (the reference-shaped ops keep their 256-thread workgroups)
    launch_waxpby_sdev(n, s->x, &s->S->alpha, s->p, s->x, stop);
    launch_waxpby_sdev(n, s->r, &s->S->neg_alpha, s->Ap, s->r, stop);
    mark(s, R_WAXPBY);
    phase_mark(s, PH_R_UPDATE);
  }
}

static void ensure_hist(sb_cg* s, int cap)
{
  if (cap <= s->hist_cap) return;
  sb_free(s->rr_hist), sb_free(s->pAp_hist);
  s->hist_cap = cap;
  s->rr_hist  = (double*)sb_malloc((size_t)cap * sizeof(double));
  s->pAp_hist = (double*)sb_malloc((size_t)cap * sizeof(double));
}

void sb_cg_start(sb_cg* s, int itermax, double eps)
{
  need_init();
  if (s->prec == 1) return sp_cg_start(s, itermax, eps);
  const uint32_t n = s->nr;
  s->started      = false;
  s->seqLatched   = -1;
  s->seqLatched   = cg_seq(s) ? 1 : 0; // the dot order, decided once per solve (cg_seq) ...
  apply_dot_order(s);                  // ... and the op list it runs
  s->fusepLatched = fusep_plan(s) ? 1 : 0; // decided once per solve (fusep_plan)
  s->foldLatched  = -1;
  s->foldLatched  = halo_fold_plan(s) ? 1 : 0; // ... and so is the folded halo exchange (halo_fold_plan)
  halo_push_watch(s->halo, &s->S->p2p_error, true);
  ensure_hist(s, itermax + 2);
  s->timing  = !s->fused; // the reference-shaped op list is the one that gets the region table
  s->evUsed  = 0;
  memset(&s->hostS, 0, sizeof s->hostS);
  s->hostS.itermax  = itermax;
  s->hostS.eps      = eps;
  s->hostS.hist_cap = s->hist_cap;
  HIP_CHECK(hipMemcpyAsync(s->S, &s->hostS, sizeof(CgScalars), hipMemcpyHostToDevice, g.stream));
  HIP_CHECK(hipMemsetAsync(s->x, 0, (size_t)n * sizeof(double), g.stream)); // x0 = 0 (:28)
  s->p = s->pbuf[0];
  HIP_CHECK(hipMemsetAsync(s->pbuf[0], 0, (size_t)s->nc * sizeof(double), g.stream));
  HIP_CHECK(hipMemsetAsync(s->pbuf[1], 0, (size_t)s->nc * sizeof(double), g.stream));
  mark(s, -1);
  // prologue, src/CGSolver.c:94-100
  launch_waxpby(n, 1.0, s->x, 0.0, s->x, s->p, nullptr);
  mark(s, R_WAXPBY);
  halo_exchange(s->halo, s->p, nullptr);
  mark(s, R_COMM);
  launch_spmv(s->A, s->p, s->Ap, nullptr, nullptr);
  mark(s, R_SPMVM);
  if (s->fused) {
    launch_dot_spans(2, n, s->b, s->Ap, nullptr, s->r, s->S, s->partials, nullptr);
    mark(s, R_WAXPBY);
  } else {
    launch_waxpby(n, 1.0, s->b, -1.0, s->Ap, s->r, nullptr);
    mark(s, R_WAXPBY);
    cg_dot(s, s->r, s->r, nullptr);
  }
  scalar_launch<0>(s, 0, nullptr);
  mark(s, R_DDOT);
  s->k_next   = 1;
  s->started  = true;
  s->betaFold = 0;
}

void sb_cg_run_iters(sb_cg* s, int iters)
{
  need_init();
  if (!s->started) SB_FATAL("sb_cg_run_iters before sb_cg_start");
  if (s->prec == 1) return sp_cg_run_iters(s, iters);
  phase_mark(s, -1);
  for (int i = 0; i < iters; i++) loop_body(s, s->k_next++);
  flush_beta_fold(s); // every call leaves the loop state complete (counters, history, stop flag)
}

// a failed wait on the peer-mapped paths ends the process with the rank in the message (both precisions).  (A rank that fails
// poisons what it would have published, so the others leave their waits at once with code 2: the rank that saw the CAUSE --
// code 1 or 3 -- is the one whose message matters.)
static void comm_failures(const sb_halo* halo, int p2pError)
{
  if (halo && halo->p2p) {
    int e = 0;
    HIP_CHECK(hipMemcpy(&e, halo->err, sizeof e, hipMemcpyDeviceToHost));
    if (e == 1)
      SB_FATAL("rank %d: a neighbour's halo block did not arrive within %lld ms (SB_P2P_TIMEOUT_MS raises the bound, "
               "SB_P2P_HALO=0 selects RCCL)", g.rank, halo->push.timeoutTicks / P2P_TICKS_PER_MS);
    if (e && p2pError != 1) p2pError = 2;
  }
  if (p2pError == 2)
    SB_FATAL("rank %d: another rank reported a communication failure over the peer-mapped paths and ended the exchange "
             "(its own message says which wait ran out); this rank stopped with it", g.rank);
  if (p2pError)
    SB_FATAL("rank %d: a peer's contribution to an in-kernel all-reduce did not arrive within %lld ms "
             "(SB_P2P_TIMEOUT_MS raises the bound, SB_P2P=0 selects the RCCL all-reduce)", g.rank,
        g.p2pTimeoutTicks / P2P_TICKS_PER_MS);
}
static void cg_comm_failures(const sb_cg* s, int p2pError) { comm_failures(s->halo, p2pError); }

// the end of a solve, both precisions (the stream is idle): the region table of a timed solve, and the latches are released
static void cg_solve_over(sb_cg* s)
{
  if (s->timing) {
    for (double& v : s->region_ms) v = 0.0;
    for (size_t i = 1; i < s->evUsed; i++) {
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, s->ev[i - 1], s->ev[i]));
      if (s->evRegion[i] >= 0) s->region_ms[s->evRegion[i]] += ms;
    }
  }
  s->timing       = false;
  s->fusepLatched = -1; // the next sb_cg_start / sp_cg_start decides anew
  s->seqLatched   = -1;
  s->foldLatched  = -1;
  apply_dot_order(s); // (a dot order or fused level asked for during the solve)
}

int sb_cg_finish(sb_cg* s)
{
  need_init();
  if (s->prec == 1) return sp_cg_finish(s);
  if (s->nr) { // the x update the last body left to "the next p update": nobody comes after it
    // (fused p update: body k left p_k in pbuf[k & 1]; which body ran last is on the device -- n_pAp -- not on the host)
    const bool fp = fusep_plan(s);
    launch_cg_x_finalize(s->nr, s->x, fp ? s->pbuf[0] : s->p, fp ? s->pbuf[1] : s->p, s->S);
    HIP_CHECK(hipMemsetAsync(&s->S->x_pending, 0, sizeof(int), g.stream));
  }
  HIP_CHECK(hipStreamSynchronize(g.stream));
  CgScalars h;
  HIP_CHECK(hipMemcpy(&h, s->S, sizeof h, hipMemcpyDeviceToHost));
  cg_comm_failures(s, h.p2p_error);
  cg_solve_over(s);
  return h.iters + 1; // the value of k when the reference's for loop exits (:107,:140)
}

int sb_cg_solve(sb_cg* s, int itermax, double eps)
{
  sb_cg_start(s, itermax, eps);
  HIP_CHECK(hipEventRecord(s->evLoop0, g.stream));
  sb_cg_run_iters(s, itermax > 1 ? itermax - 1 : 0);
  HIP_CHECK(hipEventRecord(s->evLoop1, g.stream));
  const int k = sb_cg_finish(s);
  HIP_CHECK(hipEventElapsedTime(&s->loop_ms, s->evLoop0, s->evLoop1));
  return k;
}

int sb_cg_history(const sb_cg* s, double* rr_out, int rr_cap, double* pAp_out, int pAp_cap, int* n_pAp)
{
  need_init();
  if (s->prec == 1) return sp_cg_history(s, rr_out, rr_cap, pAp_out, pAp_cap, n_pAp);
  HIP_CHECK(hipStreamSynchronize(g.stream));
  CgScalars h;
  HIP_CHECK(hipMemcpy(&h, s->S, sizeof h, hipMemcpyDeviceToHost));
  int nrr = h.n_rr < s->hist_cap ? h.n_rr : s->hist_cap;
  int npa = h.n_pAp < s->hist_cap ? h.n_pAp : s->hist_cap;
  if (nrr > rr_cap) nrr = rr_cap;
  if (npa > pAp_cap) npa = pAp_cap;
  if (nrr > 0) HIP_CHECK(hipMemcpy(rr_out, s->rr_hist, (size_t)nrr * sizeof(double), hipMemcpyDeviceToHost));
  if (npa > 0) HIP_CHECK(hipMemcpy(pAp_out, s->pAp_hist, (size_t)npa * sizeof(double), hipMemcpyDeviceToHost));
  if (n_pAp) *n_pAp = npa;
  return nrr;
}

void sb_cg_solution(const sb_cg* s, double* x_host)
{
  need_init();
  if (s->prec == 1) SB_FATAL("sb_cg_solution on a single-precision solver: use sb_cg_solution_f32");
  download_original(s->A, s->x, x_host);
}

double sb_cg_check_residual(const sb_cg* s)
{
  need_init();
  if (s->prec == 1) return sp_cg_check_residual(s);
  if (!s->xexact || s->nr == 0) return 0.0;
  double m = max_abs_diff_host(s->nr, s->x, s->xexact);
  if (multi_rank()) { // commReduction(&residual, MAX), src/CGSolver.c:55
    sb_h2d(g.scalar, &m, sizeof m);
    sb_comm_reduction(g.scalar, 0);
    sb_d2h(&m, g.scalar, sizeof m);
  }
  return m;
}

double sb_debug_stream_read_gbs(size_t bytes, int reps)
{ // raw read ceiling of this device: `reps` passes over a `bytes`-sized buffer
  need_init();
  double2* buf = nullptr;
  HIP_CHECK(hipMalloc(&buf, bytes));
  HIP_CHECK(hipMemsetAsync(buf, 0, bytes, g.stream));
  const size_t n2 = bytes / sizeof(double2);
  dim3 grid((unsigned)g.prop.multiProcessorCount * 8), block(256);
  hipLaunchKernelGGL(stream_read_k, grid, block, 0, g.stream, buf, n2, g.scalar);
  hipEvent_t a, b;
  HIP_CHECK(hipEventCreate(&a));
  HIP_CHECK(hipEventCreate(&b));
  HIP_CHECK(hipEventRecord(a, g.stream));
  for (int r = 0; r < reps; r++) hipLaunchKernelGGL(stream_read_k, grid, block, 0, g.stream, buf, n2, g.scalar);
  HIP_CHECK(hipEventRecord(b, g.stream));
  HIP_CHECK(hipEventSynchronize(b));
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, a, b));
  HIP_CHECK(hipEventDestroy(a));
  HIP_CHECK(hipEventDestroy(b));
  HIP_CHECK(hipFree(buf));
  return (double)bytes * reps / (ms * 1e-3) / 1e9;
}

double sb_cg_loop_ms(const sb_cg* s) { return (double)s->loop_ms; }

void sb_cg_region_ms(const sb_cg* s, double out[4])
{
  for (int i = 0; i < 4; i++) out[i] = s->region_ms[i];
}

// --- blocking test entries: the loop's vector and scalar kernels alone, launched by the loop's own launch functions -------------
void sb_cg_update_p_launch(uint32_t n, uint32_t out[3])
{
  need_init();
  out[0] = cg_update_p_grid(n), out[1] = cg_vec_block(), out[2] = (uint32_t)g.prop.multiProcessorCount;
}
void sb_cg_update_r_launch(uint32_t n, int mode, uint32_t out[3])
{
  need_init();
  if (mode < 0 || mode > 2) SB_FATAL("sb_cg_update_r_launch: mode = %d outside 0 .. 2", mode);
  out[0] = cg_update_r_grid(n, mode), out[1] = cg_vec_block(), out[2] = (uint32_t)g.prop.multiProcessorCount;
}

// The control block of a test entry: the caller's plain data (include/sbhip.h: d[9], i[11] in CgScalars' order) uploaded between
// two runs of guard words, downloaded again field by field behind the launch.  Nothing in between is computed here.
namespace {
enum { CG_BLK_GUARD = 64 }; // guard words (8 bytes each) in front of the block and behind it
struct CgTestBlock {
  std::vector<unsigned long long> up;
  char* raw    = nullptr;
  CgScalars* S = nullptr;
  CgTestBlock(const double* d, const int* i)
  {
    static_assert(sizeof(CgScalars) % 8 == 0, "the guard words follow the block without a gap");
    CgScalars h = zeroed<CgScalars>();
    h.rr = d[0], h.rr_old = d[1], h.pAp = d[2], h.alpha = d[3], h.beta = d[4], h.neg_alpha = d[5], h.local = d[6], h.eps = d[7], h.snap_rr = d[8];
    h.stop = i[0], h.stop_next = i[1], h.iters = i[2], h.n_rr = i[3], h.n_pAp = i[4], h.itermax = i[5], h.hist_cap = i[6];
    h.x_pending = i[7], h.p2p_error = i[8], h.snap_iters = i[9], h.snap_stop_next = i[10];
    up.resize(2 * CG_BLK_GUARD + sizeof h / 8);
    for (size_t k = 0; k < up.size(); k++) up[k] = 0x7FF8C0DE00000000ull | k; // quiet NaNs with a payload
    memcpy(&up[CG_BLK_GUARD], &h, sizeof h);
    raw = (char*)sb_malloc(up.size() * 8);
    HIP_CHECK(hipStreamSynchronize(g.stream));
    HIP_CHECK(hipMemcpy(raw, up.data(), up.size() * 8, hipMemcpyHostToDevice));
    S = reinterpret_cast<CgScalars*>(raw + 8 * CG_BLK_GUARD);
  }
  // waits for the launch; every field back into d / i; returns the number of guard words that changed
  int done(double* d, int* i)
  {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(g.stream));
    std::vector<unsigned long long> back(up.size());
    HIP_CHECK(hipMemcpy(back.data(), raw, back.size() * 8, hipMemcpyDeviceToHost));
    sb_free(raw);
    int changed = 0;
    for (size_t k = 0; k < back.size(); k++)
      if ((k < CG_BLK_GUARD || k >= back.size() - CG_BLK_GUARD) && back[k] != up[k]) changed++;
    CgScalars h;
    memcpy(&h, &back[CG_BLK_GUARD], sizeof h);
    d[0] = h.rr, d[1] = h.rr_old, d[2] = h.pAp, d[3] = h.alpha, d[4] = h.beta, d[5] = h.neg_alpha, d[6] = h.local, d[7] = h.eps, d[8] = h.snap_rr;
    i[0] = h.stop, i[1] = h.stop_next, i[2] = h.iters, i[3] = h.n_rr, i[4] = h.n_pAp, i[5] = h.itermax, i[6] = h.hist_cap;
    i[7] = h.x_pending, i[8] = h.p2p_error, i[9] = h.snap_iters, i[10] = h.snap_stop_next;
    return changed;
  }
};
void cg_need_fold_block(int mode, const char* fn)
{
  if (mode < 0 || mode > 2) SB_FATAL("%s: mode = %d outside 0 .. 2", fn, mode);
  if (mode && cg_vec_block() != 1024u) SB_FATAL("%s: the folded scalar steps need 1024-thread workgroups (SB_VEC_BLOCK = %u)", fn, cg_vec_block());
}
} // namespace

int sb_cg_update_p_native(int mode, uint32_t n, const double* r_dev, double* p_dev, double* x_dev, int which, uint32_t m, const double* l1_dev,
    double* rr_hist_dev, double* blk_d, int* blk_i)
{
  need_init();
  cg_need_fold_block(mode, "sb_cg_update_p_native");
  if (mode && which) SB_FATAL("sb_cg_update_p_native: mode %d takes which = 0 only", mode);
  need_aligned16({ r_dev, p_dev, x_dev }, "sb_cg_update_p_native", "vectors");
  CgTestBlock b(blk_d, blk_i);
  launch_cg_update_p(mode, n, r_dev, p_dev, x_dev, b.S, which, m, l1_dev, rr_hist_dev);
  return b.done(blk_d, blk_i);
}

int sb_cg_update_r_native(int mode, uint32_t n, const double* Ap_dev, double* r_dev, double* l1out_dev, uint32_t m, const double* l1in_dev,
    double* rr_hist_dev, double* pAp_hist_dev, double* blk_d, int* blk_i)
{
  need_init();
  cg_need_fold_block(mode, "sb_cg_update_r_native");
  need_aligned16({ Ap_dev, r_dev }, "sb_cg_update_r_native", "vectors");
  CgTestBlock b(blk_d, blk_i);
  launch_cg_update_r(mode, n, Ap_dev, r_dev, b.S, l1out_dev, &b.S->stop, m, l1in_dev, rr_hist_dev, pAp_hist_dev);
  return b.done(blk_d, blk_i);
}

int sb_cg_scalar_native(int mode, int reduce, uint32_t m, const double* q_dev, double* rr_hist_dev, double* pAp_hist_dev, int to_local, int defer_x,
    int l1, double* blk_d, int* blk_i)
{
  need_init();
  if (mode < 0 || mode > 2) SB_FATAL("sb_cg_scalar_native: mode = %d outside 0 .. 2", mode);
  need_aligned16({ q_dev }, "sb_cg_scalar_native", "partials");
  CgTestBlock b(blk_d, blk_i);
  launch_cg_scalar(mode, reduce != 0, m, q_dev, b.S, rr_hist_dev, pAp_hist_dev, to_local, defer_x, l1);
  return b.done(blk_d, blk_i);
}

int sb_cg_x_finalize_native(uint32_t n, double* x_dev, const double* p0_dev, const double* p1_dev, double* blk_d, int* blk_i)
{
  need_init();
  CgTestBlock b(blk_d, blk_i);
  launch_cg_x_finalize(n, x_dev, p0_dev, p1_dev, b.S);
  return b.done(blk_d, blk_i);
}

int sb_cg_dot_spans_native(int op, uint32_t n, const double* a_dev, const double* b_dev, double* x_dev, double* r_dev, double* partials_dev,
    double* blk_d, int* blk_i)
{
  need_init();
  if (op != 1 && op != 2) SB_FATAL("sb_cg_dot_spans_native: op = %d, expected 1 or 2 (op 0 is sb_ddot_partials)", op);
  CgTestBlock b(blk_d, blk_i);
  launch_dot_spans(op, n, a_dev, b_dev, x_dev, r_dev, b.S, partials_dev, &b.S->stop);
  return b.done(blk_d, blk_i);
}

int sb_waxpby_sdev_native(uint32_t n, const double* x_dev, int negative, const double* y_dev, double* w_dev, double* blk_d, int* blk_i)
{
  need_init();
  need_aligned16({ x_dev, y_dev, w_dev }, "sb_waxpby_sdev_native", "vectors");
  CgTestBlock b(blk_d, blk_i);
  launch_waxpby_sdev(n, x_dev, negative ? &b.S->neg_alpha : &b.S->alpha, y_dev, w_dev, &b.S->stop);
  return b.done(blk_d, blk_i);
}
