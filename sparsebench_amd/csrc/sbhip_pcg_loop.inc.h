// sbhip_pcg_loop.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): the loop
// of preconditioned CG and the one place that asks how the handle's z is made: the diagonal (riding in the r
// update), the sweeps (sbhip_sgs.inc.h), the V-cycle (sbhip_mg.inc.h, sbhip_mg_fw.inc.h) or the
// Chebyshev polynomial (sbhip_poly.inc.h), alone or as the smoother of a V-cycle (sbhip_mg_poly.inc.h).
// Included behind those files, so nothing here is declared ahead of its definition; the handle is sbhip_pcg.inc.h's.
// ===========================================================================
// preconditioned CG: z and the loop
// ===========================================================================
int sb_pcg_precond(const sb_pcg* s) { return s->mgp ? 5 : s->poly ? 4 : s->mg ? (s->mg->fw ? 3 : 2) : s->sgs ? 1 : 0; }

// z = M^-1 r with the handle's preconditioner: r o dinv, the sweeps of its matrix, or the V-cycle around them (t: the forward
// sums of level 0; the diagonal does not touch it), or the polynomial on the handle's own d and w
static void precond_apply(const sb_pcg* s, const double* r, double* t, double* z, const int* stop)
{
  if (s->mgp) return mgp_apply(s, r, z, stop, false, nullptr);
  if (s->poly) return poly_apply(s->A, (const double*)s->dinv, s->poly->c, r, z, s->poly->d, s->poly->w, stop);
  if (s->mg) return mg_apply(s, r, t, z, stop);
  if (s->sgs) return sgs_apply(s->sgs, (const double*)s->dinv, r, t, z, stop);
  if (!s->nr) return;
  hipLaunchKernelGGL(precond_diag_k, dim3(stream_grid(s->nr, 256)), dim3(256), 0, g.stream, s->nr, r, (const double*)s->dinv, z);
  HIP_CHECK(hipGetLastError());
}

// the r update (PRO 1: the prologue's b - Ap) with the r.r values, z and the r.z values.  The diagonal: all of it in
// pcg_update_r_k.  Sweeps and V-cycle: the r update without z, the apply, r.z by dot_l1_k.  The polynomial: step 1 in
// poly_update_r_k, the steps behind it by poly_steps, the last of them with the r.z values.  The Chebyshev-smoothed cycle: level
// 0's step 1 in poly_update_r_k, the rest by mgp_apply, whose last kernel on level 0 makes the r.z values
template <int PRO> static void pcg_residual_and_z(sb_pcg* s)
{
  const uint32_t n = s->nr;
  if (!n) return;
  const int* stop   = &s->S->stop; // (0 throughout the prologue: sb_pcg_start has just written the block)
  const double* src = PRO ? s->b : s->r;
  const dim3 grid(vec_stream_grid(n)), block(1024);
  if (s->mgp) {
    const MgPolyLevel& V = s->mgp->lev[0];
    if (s->mgp->lev.size() == 1 && V.c.steps == 1)
      hipLaunchKernelGGL((poly_update_r_k<PRO, 1>), grid, block, 0, g.stream, n, (const double*)s->Ap, src, s->r, (const double*)s->dinv,
          V.d, s->z, V.c.c1, (const PcgScalars*)s->S, s->l1rz, s->l1rr);
    else
      hipLaunchKernelGGL((poly_update_r_k<PRO, 0>), grid, block, 0, g.stream, n, (const double*)s->Ap, src, s->r, (const double*)s->dinv,
          V.d, s->z, V.c.c1, (const PcgScalars*)s->S, s->l1rz, s->l1rr);
    mgp_apply(s, s->r, s->z, stop, true, s->l1rz);
  } else if (s->poly) {
    const PolyPlan* P = s->poly;
    if (P->c.steps == 1)
      hipLaunchKernelGGL((poly_update_r_k<PRO, 1>), grid, block, 0, g.stream, n, (const double*)s->Ap, src, s->r, (const double*)s->dinv,
          P->d, s->z, P->c.c1, (const PcgScalars*)s->S, s->l1rz, s->l1rr);
    else
      hipLaunchKernelGGL((poly_update_r_k<PRO, 0>), grid, block, 0, g.stream, n, (const double*)s->Ap, src, s->r, (const double*)s->dinv,
          P->d, s->z, P->c.c1, (const PcgScalars*)s->S, s->l1rz, s->l1rr);
    poly_steps(s->A, (const double*)s->dinv, P->c, s->r, s->z, P->d, P->w, stop, s->l1rz);
  } else if (!s->sgs) {
    hipLaunchKernelGGL(pcg_update_r_k<PRO>, grid, block, 0, g.stream, n, (const double*)s->Ap, src, s->r, (const double*)s->dinv, s->z,
        (const PcgScalars*)s->S, s->l1rz, s->l1rr);
  } else {
    hipLaunchKernelGGL(sgs_update_r_k<PRO>, grid, block, 0, g.stream, n, (const double*)s->Ap, src, s->r, (const PcgScalars*)s->S,
        s->l1rr);
    precond_apply(s, s->r, s->sgs->t, s->z, stop);
    hipLaunchKernelGGL(dot_l1_k, grid, block, 0, g.stream, n, (const double*)s->r, (const double*)s->z, s->l1rz, stop);
  }
  HIP_CHECK(hipGetLastError());
}

// bytes one apply reads and writes.  Diagonal: r, dinv in, z out.  SGS: sgs_bytes.  MG: mg_bytes.  Polynomial: poly_bytes.
// Chebyshev-smoothed cycle: mgp_bytes
double sb_pcg_precond_bytes(const sb_pcg* s)
{
  if (s->mgp) return mgp_bytes(s);
  if (s->poly) return poly_bytes(s);
  if (!s->sgs) return 24.0 * (double)s->nr;
  return s->mg ? mg_bytes(s) : sgs_bytes(s->sgs, s->nr);
}

// The two probes run applies outside a solve on scratch vectors of their own, allocated and freed by the call (t: the forward
// sums, which the diagonal leaves alone)
void sb_pcg_apply_precond(sb_pcg* s, const double* r_host, double* z_host)
{
  need_init();
  if (s->clock.open) SB_FATAL("sb_pcg_apply_precond between sb_pcg_start and sb_pcg_finish: the solve's vectors are in flight");
  if (!s->nr) return;
  const size_t nb = (size_t)s->nr * sizeof(double) + 4096;
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
  const size_t nb = (size_t)s->nr * sizeof(double) + 4096;
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
  mgp_release(s);
  poly_release(s);
  mg_release(s);
  sgs_release(s);
  sb_free(s->r), sb_free(s->z), sb_free(s->p), sb_free(s->Ap), sb_free(s->x), sb_free(s->b), sb_free(s->dinv), sb_free(s->xexact);
  sb_free(s->S), sb_free(s->l1pAp), sb_free(s->l1rz), sb_free(s->l1rr), sb_free(s->rr_hist), sb_free(s->rz_hist), sb_free(s->pAp_hist);
  delete s;
}

// launches per loop body: p update | SpMV (+ p.Ap values) | alpha | r update (+ z, r.z and r.r values) | beta = 5 where the
// selected SpMV kernel has a fused dot; native CRS and generic C add the dot pass: 6.  An SGS handle: the r update makes no z;
// nC forward and nC - 1 backward launches and the r.z pass stand in between it and beta: 2 nC + 5 (+ 1).  An MG handle: the
// V-cycle's launches in the sweeps' place: 6 (+ 1) + mg_apply_launches.  A polynomial handle: step 1 rides in the r update, the
// last step makes the r.z values; an SpMV and a step kernel per step behind the first: 5 (+ 1) + 2 (steps - 1).  A
// Chebyshev-smoothed cycle: the r update counts among the cycle's launches and no r.z pass follows: 4 (+ 1) + mgp_apply_launches
int sb_pcg_launches_per_body(const sb_pcg* s)
{
  if (s->mgp) return (spmv_dot_kind(s->A) ? 4 : 5) + mgp_apply_launches(s);
  if (s->poly) return (spmv_dot_kind(s->A) ? 5 : 6) + 2 * (s->poly->c.steps - 1);
  if (s->mg) return (spmv_dot_kind(s->A) ? 6 : 7) + mg_apply_launches(s);
  return (spmv_dot_kind(s->A) ? 5 : 6) + (s->sgs ? 2 * sb_pcg_colours(s) : 0);
}

template <int MODE> static void pcg_scalar_launch(sb_pcg* s)
{
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
  // prologue: x0 = 0, p = 1.0 x + 0.0 x = 0, Ap = A p, r = 1.0 b + (-1.0) Ap, z = r o dinv, r.r, r.z, the loop test for k = 1
  HIP_CHECK(hipMemsetAsync(s->x, 0, (size_t)s->nr * sizeof(double), g.stream));
  HIP_CHECK(hipMemsetAsync(s->p, 0, (size_t)s->nc * sizeof(double), g.stream));
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
  return read_block(s->S).iters + 1; // the value of k when the for loop exits
}

int sb_pcg_solve(sb_pcg* s, int itermax, double eps)
{
  sb_pcg_start(s, itermax, eps);
  sb_pcg_run_iters(s, loop_bodies(itermax));
  return sb_pcg_finish(s);
}
