// sbhip_poly.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): the Chebyshev
// polynomial preconditioner of PCG (kernels: poly.hip.h).  The handle is an sb_pcg whose `poly` plan is set: the
// loop, its control block, histories and every other sb_pcg_* call are sbhip_pcg.inc.h's; what differs is how z is made (step 1
// in the r update, then steps - 1 times the matrix's selected SpMV and poly_step_k, the last of them with the r.z values:
// sbhip_pcg_loop.inc.h).  No colouring, no structure of its own, no matrix download.
// ===========================================================================
// Chebyshev polynomial preconditioner
// ===========================================================================
#define SB_POLY_MAX_STEPS 16
// what the apply needs beside the matrix and dinv: host doubles, computed once (poly_coeffs)
struct PolyCoef {
  int steps = 0;
  double lmax = 0.0, lmin = 0.0, c1 = 0.0;
  double a[SB_POLY_MAX_STEPS + 1] = { 0.0 }, b[SB_POLY_MAX_STEPS + 1] = { 0.0 }; // a[j], b[j] of step j = 2 .. steps
};
struct PolyPlan {
  PolyCoef c;
  double *d = nullptr, *w = nullptr; // the recurrence's direction and A z; device row order
  std::vector<double> g;             // the bound's row values, device row order
};

// the contract's coefficients, in exactly its order of operations
static PolyCoef poly_coeffs(int steps, double lmax, double ratio)
{
  PolyCoef c;
  c.steps = steps, c.lmax = lmax;
  c.lmin             = lmax / ratio;
  const double theta = (c.lmax + c.lmin) * 0.5;
  const double delta = (c.lmax - c.lmin) * 0.5;
  const double sigma = theta / delta;
  c.c1               = 1.0 / theta;
  double rho         = 1.0 / sigma;
  for (int j = 2; j <= steps; j++) {
    const double rj = 1.0 / (2.0 * sigma - rho);
    c.a[j]          = rj * rho;
    c.b[j]          = (2.0 * rj) / delta;
    rho             = rj;
  }
  return c;
}

// steps 2 .. steps of the apply behind step 1 (z = d = (r o dinv) * c1 already made): w = A z by the selected SpMV without a fused
// dot, then poly_step_k.  l1rz != NULL: the last step leaves the level-1 values of r.z there
static void poly_steps(const sb_matrix* m, const double* dinv, const PolyCoef& c, const double* r, double* z, double* d, double* w,
    const int* stop, double* l1rz)
{
  const uint32_t n = m->nr;
  if (!n) return;
  const dim3 grid(vec_stream_grid(n)), block(1024);
  for (int j = 2; j <= c.steps; j++) {
    launch_spmv(m, z, w, nullptr, stop);
    if (j == c.steps && l1rz)
      hipLaunchKernelGGL(poly_step_k<1>, grid, block, 0, g.stream, n, r, (const double*)w, dinv, d, z, c.a[j], c.b[j], l1rz, stop);
    else
      hipLaunchKernelGGL(poly_step_k<0>, grid, block, 0, g.stream, n, r, (const double*)w, dinv, d, z, c.a[j], c.b[j], (double*)nullptr,
          stop);
  }
  HIP_CHECK(hipGetLastError());
}
// z = M^-1 r, a function of the matrix, dinv and the coefficients, not of a handle: a V-cycle can call it per level.  z is an SpMV
// operand (nc entries and the padding the SpMV kernels expect); d, w: nr doubles
static void poly_apply(const sb_matrix* m, const double* dinv, const PolyCoef& c, const double* r, double* z, double* d, double* w,
    const int* stop)
{
  const uint32_t n = m->nr;
  if (!n) return;
  hipLaunchKernelGGL(poly_first_k, dim3(stream_grid(n, 256)), dim3(256), 0, g.stream, n, r, dinv, d, z, c.c1, stop);
  HIP_CHECK(hipGetLastError());
  poly_steps(m, dinv, c, r, z, d, w, stop, nullptr);
}

// g in the device's row order, computed on the device from dinv
static std::vector<double> poly_rowbound(const sb_matrix* m, const double* dinv_dev)
{
  std::vector<double> h(m->nr);
  if (!m->nr) return h;
  double* gd = scratch_ws(0, m->nr);
  const dim3 grid((m->nr + 255) / 256), block(256);
  if (m->fmt == 0) hipLaunchKernelGGL(poly_bound_crs_k, grid, block, 0, g.stream, m->nr, m->rowPtr, m->colInd, m->val, dinv_dev, gd);
  else
    hipLaunchKernelGGL(poly_bound_scs_k, grid, block, 0, g.stream, m->nr, m->C, m->chunkPtr, m->chunkLens, m->colInd, m->val, dinv_dev,
        gd);
  HIP_CHECK(hipGetLastError());
  sb_d2h(h.data(), gd, h.size() * sizeof(double));
  return h;
}

sb_pcg* sb_pcg_create_poly(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int steps, double lmax,
    double ratio)
{
  const char* fn = "sb_pcg_create_poly";
  if (steps < 1 || steps > SB_POLY_MAX_STEPS) SB_FATAL("%s: steps = %d: the polynomial has 1 to %d steps", fn, steps, SB_POLY_MAX_STEPS);
  if (ratio == 0.0) ratio = 16.0;
  if (!(ratio > 1.0 && ratio < INFINITY)) SB_FATAL("%s: ratio = %g: lmax / lmin must be finite and greater than 1", fn, ratio);
  if (!(lmax < INFINITY)) SB_FATAL("%s: lmax = %g: the caller's lmax must be finite (0.0 or less: the bound)", fn, lmax);
  sb_pcg* s   = pcg_create(m, halo, b_host, xexact_host, nullptr, fn, "Chebyshev polynomial");
  PolyPlan* P = new PolyPlan();
  s->poly     = P;
  P->g        = poly_rowbound(m, s->dinv);
  if (!(lmax > 0.0)) {
    lmax = 0.0;
    for (double v : P->g) {
      if (!(v > 0.0 && v < INFINITY)) { // a NaN would otherwise drop out of the maximum
        lmax = v;
        break;
      }
      if (v > lmax) lmax = v;
    }
    if (!(lmax > 0.0 && lmax < INFINITY))
      SB_FATAL("%s: lmax = %g: the bound on the largest eigenvalue of D^-1 A (the largest absolute row sum of D^-1/2 A D^-1/2) is "
               "not finite and positive; pass lmax", fn, lmax);
  }
  P->c = poly_coeffs(steps, lmax, ratio);
  if (!(P->c.c1 > 0.0 && P->c.c1 < INFINITY)) SB_FATAL("%s: lmax = %g, ratio = %g: 1 / theta is not finite and positive", fn, lmax, ratio);
  const size_t nb = (size_t)m->nr * sizeof(double) + 4096;
  P->d = (double*)sb_malloc(nb), P->w = (double*)sb_malloc(nb);
  HIP_CHECK(hipStreamSynchronize(g.stream));
  return s;
}

static void poly_release(sb_pcg* s)
{
  if (!s->poly) return;
  sb_free(s->poly->d), sb_free(s->poly->w);
  delete s->poly;
  s->poly = nullptr;
}

static const PolyPlan* need_poly(const sb_pcg* s, const char* fn)
{
  if (!s->poly) SB_FATAL("%s: the handle has another preconditioner (sb_pcg_create_poly makes the polynomial one)", fn);
  return s->poly;
}
static int mgp_steps(const sb_pcg* s); // (sbhip_mg_poly.inc.h)
int sb_pcg_poly_steps(const sb_pcg* s) { return s->poly ? s->poly->c.steps : s->mgp ? mgp_steps(s) : 0; }
void sb_pcg_poly_interval(const sb_pcg* s, double out[2])
{
  const PolyPlan* P = need_poly(s, "sb_pcg_poly_interval");
  out[0] = P->c.lmin, out[1] = P->c.lmax;
}
void sb_pcg_poly_coeffs(const sb_pcg* s, double* out)
{
  const PolyPlan* P = need_poly(s, "sb_pcg_poly_coeffs");
  out[0]            = P->c.c1;
  for (int j = 2; j <= P->c.steps; j++) out[2 * j - 3] = P->c.a[j], out[2 * j - 2] = P->c.b[j];
}
void sb_pcg_poly_rowbound(const sb_pcg* s, double* g_host)
{
  need_init();
  const PolyPlan* P               = need_poly(s, "sb_pcg_poly_rowbound");
  const std::vector<uint32_t> o2n = old_to_device_rows(s->A);
  for (uint32_t i = 0; i < s->A->nr; i++) g_host[i] = P->g[o2n[i]];
}

// bytes one apply reads and writes: per step behind the first the SpMV (sb_matrix_spmv_bytes) and poly_step_k's 56 B per row; the
// first step's dinv in, d and z out of the r update: 24 B per row
static double poly_bytes(const sb_pcg* s)
{
  return (double)(s->poly->c.steps - 1) * ((double)sb_matrix_spmv_bytes(s->A) + 56.0 * (double)s->nr) + 24.0 * (double)s->nr;
}

// grid of poly_step_k (and poly_update_r_k) over n rows: vec_stream_grid
void sb_pcg_poly_step_launch(uint32_t n, uint32_t out[3])
{
  need_init();
  out[0] = vec_stream_grid(n), out[1] = 1024u, out[2] = (uint32_t)g.prop.multiProcessorCount;
}

void sb_pcg_poly_update_r_native(uint32_t n, int pro, int last, double nalpha, double c1, const double* Ap_dev, double* r_dev,
    const double* dinv_dev, double* d_dev, double* z_dev, double* l1_rz_dev, double* l1_rr_dev)
{
  need_init();
  if (n == 0) return;
  need_aligned16({ Ap_dev, r_dev, dinv_dev, d_dev, z_dev }, "sb_pcg_poly_update_r_native", "vectors");
  PcgScalars h  = zeroed<PcgScalars>();
  h.neg_alpha   = nalpha;
  PcgScalars* S = test_block(h);
  const dim3 grid(vec_stream_grid(n)), block(1024);
#define POLY_UR(P, L)                                                                                                       \
  hipLaunchKernelGGL((poly_update_r_k<P, L>), grid, block, 0, g.stream, n, Ap_dev, (const double*)r_dev, r_dev, dinv_dev, d_dev, \
      z_dev, c1, (const PcgScalars*)S, l1_rz_dev, l1_rr_dev)
  if (pro && last) POLY_UR(1, 1);
  else if (pro) POLY_UR(1, 0);
  else if (last) POLY_UR(0, 1);
  else POLY_UR(0, 0);
#undef POLY_UR
  test_block_done(S);
}

void sb_pcg_poly_step_native(uint32_t n, int last, double a, double b, const double* r_dev, const double* w_dev, const double* dinv_dev,
    double* d_dev, double* z_dev, double* l1_rz_dev)
{
  need_init();
  if (n == 0) return;
  need_aligned16({ r_dev, w_dev, dinv_dev, d_dev, z_dev }, "sb_pcg_poly_step_native", "vectors");
  const dim3 grid(vec_stream_grid(n)), block(1024);
  if (last) hipLaunchKernelGGL(poly_step_k<1>, grid, block, 0, g.stream, n, r_dev, w_dev, dinv_dev, d_dev, z_dev, a, b, l1_rz_dev, zero_flag());
  else hipLaunchKernelGGL(poly_step_k<0>, grid, block, 0, g.stream, n, r_dev, w_dev, dinv_dev, d_dev, z_dev, a, b, l1_rz_dev, zero_flag());
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(g.stream));
}
