// sbhip_gmres_precond.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context):
// right-preconditioned GMRES(m).  The loop is sbhip_gmres.inc.h's, run on A M^-1 by a change of variable: the
// handle's x is u, xs = M^-1 u is the solution, and zh = M^-1 V[j] is what the step's SpMV reads.  M^-1 is a diagonal (the
// handle's own copy of a plan-less sb_pcg handle's dinv, or the caller's) or the plan of a borrowed sb_pcg handle: the handle's
// RightPrecond (sbhip_solver.inc.h, sbhip_mg.inc.h), which BiCGStab holds too.  Double precision, one rank, tree dot order.
// ===========================================================================
// GMRES on A M^-1
// ===========================================================================
// M's preconditioner on the right of A.  M is borrowed: it must outlive the handle, be made over the same matrix, and have no
// solve open here or at any sb_gmres_start.  A diagonal M without a plan: its dinv is copied and M is not referred to afterwards
sb_gmres* sb_gmres_create_pre(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int restart,
    const sb_pcg* M)
{
  need_init();
  need_dp(m, "sb_gmres_create_pre", "GMRES");
  need_tree("sb_gmres_create_pre", "preconditioned GMRES", "sb_cg");
  RightPrecond::need_borrowable(m, M, "sb_gmres_create_pre");
  (void)halo;
  sb_gmres* s     = gm_create(m, b_host, xexact_host, restart, "sb_gmres_create_pre");
  const size_t vb = s->ldv * sizeof(double) + 4096;
  s->zh = (double*)sb_malloc(vb), s->xs = (double*)sb_malloc(vb);
  HIP_CHECK(hipMemsetAsync(s->zh, 0, vb, g.stream));
  HIP_CHECK(hipMemsetAsync(s->xs, 0, vb, g.stream));
  s->pre.borrow(M, vb);
  HIP_CHECK(hipStreamSynchronize(g.stream));
  return s;
}

// the caller's diagonal on the right of A: nr finite non-zero doubles of either sign in original row order (a PCG handle takes
// positive ones only, so this diagonal has an entry point of its own)
sb_gmres* sb_gmres_create_dinv(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int restart,
    const double* dinv_host)
{
  need_init();
  need_dp(m, "sb_gmres_create_dinv", "GMRES");
  need_tree("sb_gmres_create_dinv", "preconditioned GMRES", "sb_cg");
  if (!dinv_host) SB_FATAL("sb_gmres_create_dinv: no dinv_host");
  for (uint32_t i = 0; i < m->nr; i++)
    if (!(dinv_host[i] != 0.0 && fabs(dinv_host[i]) < INFINITY))
      SB_FATAL("sb_gmres_create_dinv: dinv[%u] = %g: the preconditioner's entries must be finite and non-zero", i, dinv_host[i]);
  (void)halo;
  sb_gmres* s     = gm_create(m, b_host, xexact_host, restart, "sb_gmres_create_dinv");
  const size_t vb = s->ldv * sizeof(double) + 4096;
  double** vecs[] = { &s->zh, &s->xs, &s->pre.dinv };
  for (double** v : vecs) {
    *v = (double*)sb_malloc(vb);
    HIP_CHECK(hipMemsetAsync(*v, 0, vb, g.stream));
  }
  HIP_CHECK(hipStreamSynchronize(g.stream));
  upload_permuted(m, dinv_host, s->pre.dinv);
  return s;
}

// -1: no preconditioner (sb_gmres_create); 0: a diagonal; else the plan's kind as sb_pcg_precond reports it
int sb_gmres_precond(const sb_gmres* s) { return s->pre.set() ? s->pre.kind() : -1; }

void sb_gmres_dinv(const sb_gmres* s, double* dinv_host)
{
  need_init();
  if (!s->pre.set()) SB_FATAL("sb_gmres_dinv: the handle has no preconditioner (sb_gmres_create)");
  download_original(s->A, s->pre.diagonal(), dinv_host); // a plan's: level 0's, the borrowed handle's
}

// --- the three riding kernels on a caller's vectors (blocking; tests), through the loop's gm_launch_* -------------------------
// mode -1: the unpreconditioned kernel (dinv, d, z unused); 0: z = out o dinv; 1: d = z = (out o dinv) * c1 (the arguments are
// checked by gm_pre_native_args, sbhip_gmres.inc.h)

// out = a / *scalar_dev, *g0_dev = *scalar_dev
void sb_gmres_pre_scale_native(uint32_t n, int mode, double c1, const double* a_dev, const double* scalar_dev, double* out_dev,
    double* g0_dev, const double* dinv_dev, double* d_dev, double* z_dev)
{
  need_init();
  gm_pre_native_args(mode, dinv_dev, d_dev, z_dev, "sb_gmres_pre_scale_native");
  if (n == 0) return;
  gm_launch_scale(n, a_dev, scalar_dev, out_dev, g0_dev, PrecondRide{ mode, dinv_dev, d_dev, c1 }, z_dev, nullptr);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(g.stream));
}

// w += c[i] * V[i], ascending i (the x update of a close)
void sb_gmres_pre_multiupdate_native(uint32_t n, int mode, double c1, int nvec, const double* V_dev, size_t ldv, const double* c_dev,
    double* w_dev, const double* dinv_dev, double* d_dev, double* z_dev)
{
  need_init();
  gm_pre_native_args(mode, dinv_dev, d_dev, z_dev, "sb_gmres_pre_multiupdate_native");
  if (nvec < 1 || ldv < n) SB_FATAL("sb_gmres_pre_multiupdate_native: nvec = %d, ldv = %zu, n = %u", nvec, ldv, n);
  gm_need_vectors(V_dev, w_dev, ldv, "sb_gmres_pre_multiupdate_native");
  if (mode >= 0) need_aligned16({ dinv_dev, d_dev, z_dev }, "sb_gmres_pre_multiupdate_native", "vectors");
  if (n == 0) return;
  gm_launch_multiadd(n, nvec, V_dev, ldv, c_dev, w_dev, PrecondRide{ mode, dinv_dev, d_dev, c1 }, z_dev, nullptr);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(g.stream));
}

// The step-and-normalise kernel at cycle position j on a throw-away state of restart length j + 1 whose rotations are zero:
// hcol_host holds the j + 1 entries of H's column before the rotations, gj is g[j], l1_dev the level-1 values of w . w over
// the (n + 255) / 256 groups.  vnext = w / hn.  out_host takes H's column (j + 1 entries), then cs[j], sn[j], g[j], g[j+1],
// the estimate and hn
void sb_gmres_pre_step_native(uint32_t n, int mode, double c1, int j, const double* hcol_host, double gj, const double* l1_dev,
    const double* w_dev, double* vnext_dev, const double* dinv_dev, double* d_dev, double* z_dev, double* out_host)
{
  need_init();
  gm_pre_native_args(mode, dinv_dev, d_dev, z_dev, "sb_gmres_pre_step_native");
  if (j < 0 || j > 1023) SB_FATAL("sb_gmres_pre_step_native: cycle position %d outside 0 .. 1023", j);
  const size_t M = (size_t)j + 1, head = (sizeof(GmScalars) + 15u) & ~(size_t)15u;
  const size_t doubles = M * (M + 1) + 3 * M + 2 * (M + 1);
  std::vector<char> h(head + doubles * sizeof(double), 0);
  GmScalars* S = reinterpret_cast<GmScalars*>(h.data());
  S->itermax = 1 << 30, S->k = 1; // (hist_cap = 0: nothing is recorded)
  double* d = reinterpret_cast<double*>(h.data() + head);
  char* dev = (char*)sb_malloc(h.size());
  double* dd = reinterpret_cast<double*>(dev + head);
  GmView gv;
  memset(&gv, 0, sizeof gv);
  gv.S = reinterpret_cast<GmScalars*>(dev), gv.m = (int)M;
  size_t o = 0;
  gv.H = dd + o, o += M * (M + 1);
  gv.cs = dd + o, o += M;
  gv.sn = dd + o, o += M;
  gv.y = dd + o, o += M;
  gv.g = dd + o, d[o + j] = gj, o += M + 1;
  gv.hcol = dd + o;
  for (size_t i = 0; i < M; i++) d[o + i] = hcol_host[i];
  HIP_CHECK(hipStreamSynchronize(g.stream));
  HIP_CHECK(hipMemcpy(dev, h.data(), h.size(), hipMemcpyHostToDevice));
  gm_launch_step(n, l1_dev, gv, j, w_dev, vnext_dev, PrecondRide{ mode, dinv_dev, d_dev, c1 }, z_dev);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(g.stream));
  HIP_CHECK(hipMemcpy(h.data(), dev, h.size(), hipMemcpyDeviceToHost));
  sb_free(dev);
  const double* Hj = d + (size_t)j * (M + 1);
  for (size_t i = 0; i < M; i++) out_host[i] = Hj[i];
  const double* gg = d + M * (M + 1) + 3 * M;
  out_host[M] = d[M * (M + 1) + j], out_host[M + 1] = d[M * (M + 1) + M + j];
  out_host[M + 2] = gg[j], out_host[M + 3] = gg[j + 1], out_host[M + 4] = S->normr, out_host[M + 5] = S->hn;
}
