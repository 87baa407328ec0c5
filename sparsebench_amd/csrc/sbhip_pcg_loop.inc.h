// sbhip_pcg_loop.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): the loop
// of preconditioned CG and the one place that asks how the handle's z is made: by the diagonal (riding in the r
// update), or by the V-cycle of the handle's plan (sbhip_mg.inc.h), smoothed by the sweeps or by the
// Chebyshev polynomial.  Included behind the plan's files, so nothing here is declared ahead of its definition; the handle is
// sbhip_pcg.inc.h's.
// ===========================================================================
// preconditioned CG: z and the loop
// ===========================================================================

// z = M^-1 r with the handle's preconditioner: r o dinv, or the cycle of its plan (t: the sweeps' forward sums of level 0; the
// diagonal and the polynomial do not touch it)
static void precond_apply(const sb_pcg* s, const double* r, double* t, double* z, const int* stop)
{
  if (s->pre) return precond_cycle(s->pre, r, t, z, stop, false, nullptr);
  if (!s->nr) return;
  hipLaunchKernelGGL(precond_diag_k, dim3(stream_grid(s->nr, 256)), dim3(256), 0, g.stream, s->nr, r, (const double*)s->dinv, z);
  HIP_CHECK(hipGetLastError());
}

// the r update (PRO 1: the prologue's b - Ap) with the r.r values, z and the r.z values.  The diagonal: all of it in
// pcg_update_r_k.  The polynomial, alone or in a cycle: level 0's step 1 in poly_update_r_k, the rest by the cycle, whose last
// kernel on level 0 makes the r.z values (one level of one step: poly_update_r_k itself).  The sweeps, alone or in a cycle: the r
// update without z, the cycle, r.z by dot_l1_k
template <int PRO> static void pcg_residual_and_z(sb_pcg* s)
{
  const uint32_t n = s->nr;
  if (!n) return;
  const int* stop      = &s->S->stop; // (0 throughout the prologue: sb_pcg_start has just written the block)
  const double* src    = PRO ? s->b : s->r;
  const PrecondPlan* M = s->pre;
  const dim3 grid(vec_stream_grid(n)), block(1024);
  if (!M) {
    hipLaunchKernelGGL(pcg_update_r_k<PRO>, grid, block, 0, g.stream, n, (const double*)s->Ap, src, s->r, (const double*)s->dinv, s->z,
        (const PcgScalars*)s->S, s->l1rz, s->l1rr);
  } else if (M->smoother == SMOOTH_CHEB) {
    const PrecondLevel& V = M->lev[0];
    if (M->lev.size() == 1 && V.cheb.c.steps == 1)
      hipLaunchKernelGGL((poly_update_r_k<PRO, 1>), grid, block, 0, g.stream, n, (const double*)s->Ap, src, s->r, (const double*)s->dinv,
          V.cheb.d, s->z, V.cheb.c.c1, (const PcgScalars*)s->S, s->l1rz, s->l1rr);
    else
      hipLaunchKernelGGL((poly_update_r_k<PRO, 0>), grid, block, 0, g.stream, n, (const double*)s->Ap, src, s->r, (const double*)s->dinv,
          V.cheb.d, s->z, V.cheb.c.c1, (const PcgScalars*)s->S, s->l1rz, s->l1rr);
    precond_cycle(M, s->r, nullptr, s->z, stop, true, s->l1rz);
  } else {
    hipLaunchKernelGGL(sgs_update_r_k<PRO>, grid, block, 0, g.stream, n, (const double*)s->Ap, src, s->r, (const PcgScalars*)s->S,
        s->l1rr);
    precond_cycle(M, s->r, M->lev[0].sgs->t, s->z, stop, false, nullptr);
    hipLaunchKernelGGL(dot_l1_k, grid, block, 0, g.stream, n, (const double*)s->r, (const double*)s->z, s->l1rz, stop);
  }
  HIP_CHECK(hipGetLastError());
}

// bytes one apply reads and writes.  The diagonal: r, dinv in, z out
double sb_pcg_precond_bytes(const sb_pcg* s) { return s->pre ? precond_cycle_bytes(s->pre) : 24.0 * (double)s->nr; }

// The two probes run applies outside a solve on scratch vectors of their own, allocated and freed by the call (t: the forward
// sums, which the diagonal leaves alone)
void sb_pcg_apply_precond(sb_pcg* s, const double* r_host, double* z_host)
{
  need_init();
  if (s->clock.open) SB_FATAL("sb_pcg_apply_precond between sb_pcg_start and sb_pcg_finish: the solve's vectors are in flight");
  if (!s->nr) return;
  const size_t nb = (size_t)s->nc * sizeof(double) + 4096; // (nc: the polynomial's z is an SpMV operand; several ranks: collective)
  double *ar = (double*)sb_malloc(nb), *at = (double*)sb_malloc(nb), *az = (double*)sb_malloc(nb);
  upload_permuted(s->A, r_host, ar);
  precond_apply(s, ar, at, az, zero_flag());
  HIP_CHECK(hipStreamSynchronize(g.stream));
  download_original(s->A, az, z_host);
  sb_free(ar), sb_free(at), sb_free(az);
}

// GPU milliseconds of one apply, the mean over `reps` back-to-back applies on the scratch vectors (r = b); for the rate tool
double sb_pcg_apply_precond_ms(sb_pcg* s, int reps)
{
  need_init();
  if (s->clock.open) SB_FATAL("sb_pcg_apply_precond_ms between sb_pcg_start and sb_pcg_finish: the solve's vectors are in flight");
  if (!s->nr || reps < 1) return 0.0;
  const size_t nb = (size_t)s->nc * sizeof(double) + 4096;
  double *ar = (double*)sb_malloc(nb), *at = (double*)sb_malloc(nb), *az = (double*)sb_malloc(nb);
  sb_d2d(ar, s->b, (size_t)s->nr * sizeof(double));
  LoopClock c;
  c.create();
  for (int i = -1; i < reps; i++) { // (i = -1: an untimed first apply)
    if (i == 0) c.begin();
    precond_apply(s, ar, at, az, zero_flag());
  }
  c.end();
  HIP_CHECK(hipStreamSynchronize(g.stream));
  c.read();
  c.destroy();
  sb_free(ar), sb_free(at), sb_free(az);
  return (double)c.ms / reps;
}

void sb_pcg_free(sb_pcg* s)
{
  if (!s) return;
  HIP_CHECK(hipStreamSynchronize(g.stream));
  s->clock.destroy();
  if (s->halo) halo_push_watch(s->halo, &s->R->p2p_error, false);
  sb_free(s->R);
  precond_release(s);
  sb_free(s->r), sb_free(s->z), sb_free(s->p), sb_free(s->Ap), sb_free(s->x), sb_free(s->b), sb_free(s->dinv), sb_free(s->xexact);
  sb_free(s->S), sb_free(s->l1pAp), sb_free(s->l1rz), sb_free(s->l1rr), sb_free(s->rr_hist), sb_free(s->rz_hist), sb_free(s->pAp_hist);
  delete s;
}

// launches per loop body: p update | SpMV (+ p.Ap values) | alpha | r update (+ z, r.z and r.r values) | beta = 5 where the
// selected SpMV kernel has a fused dot; native CRS and generic C add the dot pass: 6.  The polynomial's plan: the r update counts
// among the cycle's launches, as level 0's step 1, and the cycle's last kernel makes the r.z values: 4 (+ 1) +
// precond_cycle_launches.  The sweeps' plan: the r update makes no z, and the r.z pass follows the cycle: 6 (+ 1) +
// precond_cycle_launches.
// Several ranks add, as sb_cg_launches_per_body counts them for CG: per halo exchange -- one for p, one per
// polynomial step behind the first -- the push and the pull (peer-mapped) or the pack kernel in front of the send / recv group;
// and, without the in-kernel all-reduce, one more kernel per scalar step (local reduce | all-reduces | step).  The all-reduce and
// send / recv calls themselves: sb_pcg_collectives_per_body
static int pcg_halo_exchanges(const sb_pcg* s) { return !s->halo ? 0 : s->pre ? s->pre->lev[0].cheb.c.steps : 1; }
int sb_pcg_launches_per_body(const sb_pcg* s)
{
  int n = spmv_dot_kind(s->A) ? 5 : 6;
  if (s->pre) n += (s->pre->smoother == SMOOTH_CHEB ? -1 : 1) + precond_cycle_launches(s->pre);
  if (!s->halo) return n;
  const sb_halo* h = s->halo;
  const int per    = halo_p2p_active(h) ? (h->totalSend ? 1 : 0) + (h->indegree ? 1 : 0) : h->totalSend ? 1 : 0;
  return n + pcg_halo_exchanges(s) * per + (p2p_dots() ? 0 : 2);
}
// communicator calls per loop body (RCCL / transport): without the peer-mapped paths 3 all-reduces (p.Ap; r.z and r.r) and a
// send / recv group per halo exchange; 0 on one rank
int sb_pcg_collectives_per_body(const sb_pcg* s)
{
  if (!s->halo) return 0;
  return (p2p_dots() ? 0 : 3) + (halo_p2p_active(s->halo) ? 0 : pcg_halo_exchanges(s));
}

template <int MODE> static void pcg_scalar_launch(sb_pcg* s)
{
  const double* qa = MODE == 2 ? s->l1pAp : s->l1rz;
  if (s->halo && p2p_dots()) { // local reduce, the in-kernel all-reduce(s) and the step in ONE launch; two values: two exchanges
    hipLaunchKernelGGL((pcg_scalar_p2p_k<MODE>), dim3(1), dim3(1024), 0, g.stream, s->nGroups, qa, (const double*)s->l1rr, s->S,
        s->rr_hist, s->rz_hist, s->pAp_hist, s->R, (const P2PView*)g.p2pView, g.p2pSeq + 1ull,
        (const int*)(s->halo->p2p ? s->halo->err : nullptr));
    HIP_CHECK(hipGetLastError());
    g.p2pSeq += MODE == 2 ? 1ull : 2ull; // (shared with sb_cg: solves of either kind alternate on one counter)
    return;
  }
  if (s->halo) { // local reduce | one all-reduce per value, in place | the step on the reduced sums
    hipLaunchKernelGGL((pcg_local_reduce_k<MODE != 2>), dim3(1), dim3(1024), 0, g.stream, s->nGroups, qa, (const double*)s->l1rr,
        (const PcgScalars*)s->S, s->R);
    HIP_CHECK(hipGetLastError());
    sb_comm_reduction(&s->R->v[0], 1);
    if (MODE != 2) sb_comm_reduction(&s->R->v[1], 1);
    hipLaunchKernelGGL((pcg_scalar_reduced_k<MODE>), dim3(1), dim3(64), 0, g.stream, s->S, (const PcgRankSums*)s->R, s->rr_hist,
        s->rz_hist, s->pAp_hist);
    HIP_CHECK(hipGetLastError());
    return;
  }
  hipLaunchKernelGGL((pcg_scalar_k<MODE>), dim3(1), dim3(1024), 0, g.stream, s->nGroups, (const double*)(MODE == 2 ? s->l1pAp : s->l1rz),
      (const double*)s->l1rr, s->S, s->rr_hist, s->rz_hist, s->pAp_hist);
  HIP_CHECK(hipGetLastError());
}

// one loop body
static void pcg_body(sb_pcg* s, int k)
{
  const uint32_t n = s->nr;
  const int* stop  = &s->S->stop;
  if (n) {
    const dim3 gridV(std::max(1u, std::min((uint32_t)g.prop.multiProcessorCount * 2u, (n / 2 + 1 + 1023u) / 1024u)));
    hipLaunchKernelGGL(pcg_update_p_k, gridV, dim3(1024), 0, g.stream, n, (const double*)s->z, s->p, s->x, (const PcgScalars*)s->S,
        k == 1 ? 1 : 0);
    HIP_CHECK(hipGetLastError());
  }
  // several ranks: p's halo tail, by the push and pull launches or by pack | send / recv.  No folded form (the fold, the push
  // inside the SpMV, the pull inside the pattern SpMV): sb_comm_halo_fold and sb_comm_halo_push_inside do not apply to PCG
  halo_exchange(s->halo, s->p, stop, nullptr, true);
  if (spmv_dot_kind(s->A)) {
    launch_spmv(s->A, s->p, s->Ap, s->l1pAp, stop);
  } else {
    launch_spmv(s->A, s->p, s->Ap, nullptr, stop);
    if (n) {
      hipLaunchKernelGGL(dot_l1_k, dim3(vec_stream_grid(n)), dim3(1024), 0, g.stream, n, (const double*)s->p, (const double*)s->Ap,
          s->l1pAp, stop);
      HIP_CHECK(hipGetLastError());
    }
  }
  pcg_scalar_launch<2>(s);
  pcg_residual_and_z<0>(s);
  pcg_scalar_launch<1>(s);
}

void sb_pcg_start(sb_pcg* s, int itermax, double eps)
{
  need_init();
  need_tree("sb_pcg_start", "PCG", "sb_cg");
  const int want = std::max(s->hist_cap, itermax + 2);
  for (double** hist : { &s->rr_hist, &s->rz_hist, &s->pAp_hist }) grow(*hist, s->hist_cap, want, 1);
  s->hist_cap  = want;
  PcgScalars h = zeroed<PcgScalars>();
  h.itermax = itermax, h.eps = eps, h.hist_cap = s->hist_cap;
  write_block(s->S, &h);
  if (s->halo) { // the push kernels of this solve look at ITS failure flag (halo_push_watch)
    HIP_CHECK(hipMemset(s->R, 0, sizeof(PcgRankSums)));
    halo_push_watch(s->halo, &s->R->p2p_error, true);
  }
  // prologue: x0 = 0, p = 1.0 x + 0.0 x = 0, Ap = A p, r = 1.0 b + (-1.0) Ap, z = r o dinv, r.r, r.z, the loop test for k = 1
  HIP_CHECK(hipMemsetAsync(s->x, 0, (size_t)s->nr * sizeof(double), g.stream));
  HIP_CHECK(hipMemsetAsync(s->p, 0, (size_t)s->nc * sizeof(double), g.stream));
  halo_exchange(s->halo, s->p, nullptr); // (as sb_cg's prologue: outside the loop's staging areas)
  launch_spmv(s->A, s->p, s->Ap, nullptr, nullptr);
  pcg_residual_and_z<1>(s);
  pcg_scalar_launch<0>(s);
  s->k_next = 1;
  s->clock.begin();
}

void sb_pcg_run_iters(sb_pcg* s, int iters)
{
  need_init();
  s->clock.need_open("sb_pcg_run_iters", "sb_pcg_start");
  for (int i = 0; i < iters; i++) pcg_body(s, s->k_next++);
}

int sb_pcg_finish(sb_pcg* s)
{
  need_init();
  s->clock.need_open("sb_pcg_finish", "sb_pcg_start");
  s->clock.end();
  if (s->nr) { // the x update the last body left to "the next p update": nobody comes after it
    hipLaunchKernelGGL(pcg_x_finalize, dim3(stream_grid(s->nr, 256)), dim3(256), 0, g.stream, s->nr, s->x, (const double*)s->p,
        (const PcgScalars*)s->S);
    hipLaunchKernelGGL(pcg_clear_pending, dim3(1), dim3(1), 0, g.stream, s->S);
    HIP_CHECK(hipGetLastError());
  }
  HIP_CHECK(hipStreamSynchronize(g.stream));
  s->clock.read();
  if (s->halo) comm_failures(s->halo, read_block(s->R).p2p_error); // a failed wait ends the process with the rank in the message
  return read_block(s->S).iters + 1; // the value of k when the for loop exits
}

int sb_pcg_solve(sb_pcg* s, int itermax, double eps)
{
  sb_pcg_start(s, itermax, eps);
  sb_pcg_run_iters(s, loop_bodies(itermax));
  return sb_pcg_finish(s);
}
