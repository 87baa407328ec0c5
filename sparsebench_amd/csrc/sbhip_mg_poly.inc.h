// sbhip_mg_poly.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): the
// Chebyshev-smoothed multigrid V-cycle of PCG (kernels: mg_poly.hip.h).  The handle is an sb_pcg whose `mgp` plan is
// set: the loop and every other sb_pcg_* call are sbhip_pcg.inc.h's; what differs is how z is made.  Per level the polynomial of
// sbhip_poly.inc.h (poly_coeffs, poly_steps, the bound) smooths before and after; between the levels stand the transfers of
// sbhip_mg_fw.inc.h (its checks, its packer, mg_prolong_p_k) with the restriction reading r and w = A z in the residual's place.
// Every SpMV is the level's selected kernel.  No SgsPlan, no colouring, no matrix download.
// ===========================================================================
// Chebyshev-smoothed V-cycle
// ===========================================================================
struct MgPolyLevel {
  MgLevel T; // A, n, dinv, r, z (level 0: the handle's dinv, the caller's r and z) and the transfers to the next level
  PolyCoef c;                        // this level's interval and coefficients; c.steps: `steps`, on the last level `coarse_steps`
  double *d = nullptr, *w = nullptr; // the recurrence's direction and A z
};
struct MgPolyPlan {
  std::vector<MgPolyLevel> lev;
  int steps = 0, coarseSteps = 0;
};

static int mgp_levels(const sb_pcg* s) { return (int)s->mgp->lev.size(); }
static uint32_t mgp_level_rows(const sb_pcg* s, int l) { return s->mgp->lev[l].T.n; }
static int mgp_steps(const sb_pcg* s) { return s->mgp->steps; }

// steps 3 and 4: w = A z by the selected SpMV, rc = omega P^T (r - w)
static void mgp_restrict(const MgPolyLevel& V, const double* r, const double* z, double* rc, const int* stop)
{
  launch_spmv(V.T.A, z, V.w, nullptr, stop);
  if (V.T.nPTChunks)
    hipLaunchKernelGGL(mgp_restrict_k, dim3((V.T.nPTChunks + 3u) / 4u), dim3(256), 0, g.stream, V.T.nPTChunks, V.T.nCoarse, V.T.PT,
        V.T.omega, r, (const double*)V.w, rc, stop);
}

// step 1 of the post-smoothing behind w = A z; l1rz != NULL: with the level-1 values of r.z
static void mgp_first(uint32_t n, const double* r, const double* w, const double* dinv, double* d, double* z, double c1, double* l1rz,
    const int* stop)
{
  if (!n) return;
  const dim3 grid(vec_stream_grid(n)), block(1024);
  if (l1rz) hipLaunchKernelGGL(mgp_first_k<1>, grid, block, 0, g.stream, n, r, w, dinv, d, z, c1, l1rz, stop);
  else hipLaunchKernelGGL(mgp_first_k<0>, grid, block, 0, g.stream, n, r, w, dinv, d, z, c1, (double*)nullptr, stop);
}

// z = V(0, r): r and z are level 0's vectors (the solve's, or sb_pcg_apply_precond's scratch), z an SpMV operand.  firstDone:
// level 0's step 1 has been made by poly_update_r_k.  l1rz != NULL: the kernel that finishes z leaves the level-1 values of r.z
// there (with one level and one step that kernel is the caller's poly_update_r_k)
static void mgp_apply(const sb_pcg* s, const double* r, double* z, const int* stop, bool firstDone, double* l1rz)
{
  const MgPolyPlan* M = s->mgp;
  const size_t L      = M->lev.size();
  for (size_t l = 0; l < L; l++) { // down: smooth from zero, restrict the residual
    const MgPolyLevel& V = M->lev[l];
    if (!V.T.n) continue;
    const double* rl = l ? V.T.r : r;
    double* zl       = l ? V.T.z : z;
    if (l || !firstDone)
      hipLaunchKernelGGL(poly_first_k, dim3(stream_grid(V.T.n, 256)), dim3(256), 0, g.stream, V.T.n, rl, (const double*)V.T.dinv, V.d, zl,
          V.c.c1, stop);
    poly_steps(V.T.A, (const double*)V.T.dinv, V.c, rl, zl, V.d, V.w, stop, L == 1 ? l1rz : nullptr);
    if (l + 1 < L) mgp_restrict(V, rl, zl, M->lev[l + 1].T.r, stop);
  }
  for (size_t l = L - 1; l-- > 0;) { // up: prolong, smooth from the guess
    const MgPolyLevel& V = M->lev[l];
    if (!V.T.n) continue;
    const double* rl = l ? V.T.r : r;
    double* zl       = l ? V.T.z : z;
    double* lz       = l ? nullptr : l1rz;
    mg_fw_prolong(V.T, M->lev[l + 1].T.z, zl, stop);
    launch_spmv(V.T.A, zl, V.w, nullptr, stop);
    mgp_first(V.T.n, rl, V.w, (const double*)V.T.dinv, V.d, zl, V.c.c1, V.c.steps == 1 ? lz : nullptr, stop);
    poly_steps(V.T.A, (const double*)V.T.dinv, V.c, rl, zl, V.d, V.w, stop, lz);
  }
  HIP_CHECK(hipGetLastError());
}

// launches of one cycle, the r update that carries level 0's step 1 among them: per level but the last 4 steps + 2 (pre-smoothing
// 2 steps - 1, the residual's SpMV, restriction, prolongation, post-smoothing 2 steps), the last 2 coarse_steps - 1
static int mgp_apply_launches(const sb_pcg* s)
{
  const int L = mgp_levels(s);
  return (L - 1) * (4 * s->mgp->steps + 2) + 2 * s->mgp->coarseSteps - 1;
}

// bytes one cycle reads and writes.  Per level but the last: 2 steps SpMVs, 2 (steps - 1) times poly_step_k's 56 B
// per row, mgp_first_k's 48, step 1's 24; both transfer structures, the restriction's two gathered fine vectors in and rc out, the
// prolongation's zc in and z in and out.  The last level as poly_bytes
static double mgp_bytes(const sb_pcg* s)
{
  double b       = 0.0;
  const size_t L = s->mgp->lev.size();
  for (size_t l = 0; l < L; l++) {
    const MgPolyLevel& V = s->mgp->lev[l];
    const double n = (double)V.T.n, spmv = (double)sb_matrix_spmv_bytes(V.T.A), st = (double)V.c.steps;
    if (l + 1 == L) {
      b += (st - 1.0) * (spmv + 56.0 * n) + 24.0 * n;
      break;
    }
    b += 2.0 * st * spmv + 2.0 * (st - 1.0) * 56.0 * n + 48.0 * n + 24.0 * n;
    b += V.T.transferBytes + 16.0 * n + 8.0 * (double)V.T.nCoarse // P^T, r and w in, rc out
         + 8.0 * (double)V.T.nCoarse + 16.0 * n;                  // P (counted above), zc in, z in and out
  }
  return b;
}

static void mgp_release(sb_pcg* s)
{
  MgPolyPlan* M = s->mgp;
  if (!M) return;
  for (size_t l = 0; l < M->lev.size(); l++) {
    MgPolyLevel& V = M->lev[l];
    mg_fw_free(V.T);
    sb_free(V.d), sb_free(V.w);
    if (l) sb_free(V.T.dinv), sb_free(V.T.r), sb_free(V.T.z); // level 0's are the handle's
  }
  delete M;
  s->mgp = nullptr;
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
  char who[64];
  snprintf(who, sizeof who, "MG-Chebyshev (level %d)", 0);
  sb_pcg* s     = pcg_create(m, halo, b_host, xexact_host, nullptr, fn, who);
  MgPolyPlan* M = new MgPolyPlan();
  M->lev.resize((size_t)nCoarse + 1);
  M->steps = steps, M->coarseSteps = coarse_steps;
  s->mgp = M;
  for (int l = 0; l <= nCoarse; l++) {
    MgPolyLevel& V = M->lev[l];
    V.T.A = l ? coarse[l - 1] : m;
    V.T.n = V.T.A->nr;
    const size_t nb = (size_t)V.T.n * sizeof(double) + 4096, nz = (size_t)V.T.A->nc * sizeof(double) + 4096;
    if (l) {
      V.T.dinv = (double*)sb_malloc(nb), V.T.r = (double*)sb_malloc(nb), V.T.z = (double*)sb_malloc(nz); // z: an SpMV operand, as p is
      HIP_CHECK(hipMemsetAsync(V.T.z, 0, nz, g.stream));
      snprintf(who, sizeof who, "MG-Chebyshev (level %d)", l);
      jacobi_dinv(V.T.A, V.T.dinv, fn, who);
    } else {
      V.T.dinv = s->dinv;
    }
    V.d = (double*)sb_malloc(nb), V.w = (double*)sb_malloc(nb);
    double lm = lmax;
    if (!(lm > 0.0)) { // this level's bound, as sb_pcg_create_poly takes it
      lm = 0.0;
      for (double v : poly_rowbound(V.T.A, V.T.dinv)) {
        if (!(v > 0.0 && v < INFINITY)) { // a NaN would otherwise drop out of the maximum
          lm = v;
          break;
        }
        if (v > lm) lm = v;
      }
      if (!(lm > 0.0 && lm < INFINITY))
        SB_FATAL("%s: level %d: lmax = %g: the bound on the largest eigenvalue of D^-1 A (the largest absolute row sum of "
                 "D^-1/2 A D^-1/2) is not finite and positive; pass lmax", fn, l, lm);
    }
    V.c = poly_coeffs(l == nCoarse ? coarse_steps : steps, lm, ratio);
    if (!(V.c.c1 > 0.0 && V.c.c1 < INFINITY))
      SB_FATAL("%s: level %d: lmax = %g, ratio = %g: 1 / theta is not finite and positive", fn, l, lm, ratio);
    if (l < nCoarse) mg_fw_transfers(V.T, coarse[l], a, l);
  }
  HIP_CHECK(hipStreamSynchronize(g.stream));
  return s;
}

static const MgPolyLevel& need_mgp_level(const sb_pcg* s, int l, const char* fn)
{
  if (!s->mgp) SB_FATAL("%s: the handle has another preconditioner (sb_pcg_create_mg_poly makes the Chebyshev-smoothed cycle)", fn);
  if (l < 0 || l >= mgp_levels(s)) SB_FATAL("%s: level %d of a handle with %d levels", fn, l, mgp_levels(s));
  return s->mgp->lev[l];
}
int sb_pcg_mg_poly_level_steps(const sb_pcg* s, int l) { return need_mgp_level(s, l, "sb_pcg_mg_poly_level_steps").c.steps; }
void sb_pcg_mg_poly_interval(const sb_pcg* s, int l, double out[2])
{
  const PolyCoef& c = need_mgp_level(s, l, "sb_pcg_mg_poly_interval").c;
  out[0] = c.lmin, out[1] = c.lmax;
}
void sb_pcg_mg_poly_coeffs(const sb_pcg* s, int l, double* out)
{
  const PolyCoef& c = need_mgp_level(s, l, "sb_pcg_mg_poly_coeffs").c;
  out[0]            = c.c1;
  for (int j = 2; j <= c.steps; j++) out[2 * j - 3] = c.a[j], out[2 * j - 2] = c.b[j];
}

// steps 4 and 6 on level l alone, on scratch vectors: rc = omega P^T (r - w), z_out = z after prolonging zc.  r, w, z and z_out
// in level l's original row order, zc and rc_out in level l + 1's
void sb_pcg_mg_poly_probe(sb_pcg* s, int l, const double* r_host, const double* w_host, const double* z_host, const double* zc_host,
    double* rc_out, double* z_out)
{
  need_init();
  const char* fn = "sb_pcg_mg_poly_probe";
  if (!s->mgp) SB_FATAL("%s: the handle has another preconditioner (sb_pcg_create_mg_poly makes the Chebyshev-smoothed cycle)", fn);
  if (s->clock.open) SB_FATAL("%s between sb_pcg_start and sb_pcg_finish: the solve's vectors are in flight", fn);
  const int L = mgp_levels(s);
  if (l < 0 || l + 1 >= L) SB_FATAL("%s: level %d of a handle with %d levels has no transfers", fn, l, L);
  const MgLevel& V = s->mgp->lev[l].T;
  const MgLevel& C = s->mgp->lev[l + 1].T;
  const size_t nf = (size_t)V.n * sizeof(double) + 4096, nc = (size_t)C.n * sizeof(double) + 4096;
  double *r = (double*)sb_malloc(nf), *w = (double*)sb_malloc(nf), *z = (double*)sb_malloc(nf);
  double *zc = (double*)sb_malloc(nc), *rc = (double*)sb_malloc(nc);
  upload_permuted(V.A, r_host, r), upload_permuted(V.A, w_host, w), upload_permuted(V.A, z_host, z), upload_permuted(C.A, zc_host, zc);
  if (V.nPTChunks)
    hipLaunchKernelGGL(mgp_restrict_k, dim3((V.nPTChunks + 3u) / 4u), dim3(256), 0, g.stream, V.nPTChunks, V.nCoarse, V.PT, V.omega,
        (const double*)r, (const double*)w, rc, zero_flag());
  mg_fw_prolong(V, zc, z, zero_flag());
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(g.stream));
  download_original(C.A, rc, rc_out), download_original(V.A, z, z_out);
  sb_free(r), sb_free(w), sb_free(z), sb_free(zc), sb_free(rc);
}

// grid of mgp_first_k over n rows: vec_stream_grid
void sb_pcg_mg_poly_first_launch(uint32_t n, uint32_t out[3])
{
  need_init();
  out[0] = vec_stream_grid(n), out[1] = 1024u, out[2] = (uint32_t)g.prop.multiProcessorCount;
}

void sb_pcg_mg_poly_first_native(uint32_t n, int last, double c1, const double* r_dev, const double* w_dev, const double* dinv_dev,
    double* d_dev, double* z_dev, double* l1_rz_dev)
{
  need_init();
  if (n == 0) return;
  need_aligned16({ r_dev, w_dev, dinv_dev, d_dev, z_dev }, "sb_pcg_mg_poly_first_native", "vectors");
  if (last && !l1_rz_dev) SB_FATAL("sb_pcg_mg_poly_first_native: last = 1 needs l1_rz_dev");
  mgp_first(n, r_dev, w_dev, dinv_dev, d_dev, z_dev, c1, last ? l1_rz_dev : nullptr, zero_flag());
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(g.stream));
}
