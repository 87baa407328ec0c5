// sbhip_poly.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): the Chebyshev
// polynomial in D^-1 A that smooths PCG's preconditioners (kernels: poly.hip.h, mg_poly.hip.h): its
// coefficients, its steps behind the first from zero and from a guess, the bound on lmax, and the kernels' test entries.  A
// function of a matrix, its dinv and the coefficients, not of a handle: which handle runs it, on which levels, is
// sbhip_mg.inc.h's.  No colouring, no structure of its own, no matrix download.
// ===========================================================================
// Chebyshev polynomial smoother
// ===========================================================================
#define SB_POLY_MAX_STEPS 16
// what the steps need beside the matrix and dinv: host doubles, computed once (poly_coeffs)
struct PolyCoef {
  int steps = 0;
  double lmax = 0.0, lmin = 0.0, c1 = 0.0;
  double a[SB_POLY_MAX_STEPS + 1] = { 0.0 }, b[SB_POLY_MAX_STEPS + 1] = { 0.0 }; // a[j], b[j] of step j = 2 .. steps
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

// steps 2 .. steps behind step 1 (z = d = (r o dinv) * c1 from zero, or mgp_first from a guess): w = A z by the selected SpMV
// without a fused dot, then poly_step_k.  z is an SpMV operand (nc entries and the padding the SpMV kernels expect); d, w: nr
// doubles.  l1rz != NULL: the last step leaves the level-1 values of r.z there.  halo != NULL (several ranks): z's
// halo tail is filled ahead of every SpMV, as sb_cg fills p's
static void poly_steps(const sb_matrix* m, const double* dinv, const PolyCoef& c, const double* r, double* z, double* d, double* w,
    const int* stop, double* l1rz, sb_halo* halo = nullptr)
{
  const uint32_t n = m->nr;
  if (!n) return;
  const dim3 grid(vec_stream_grid(n)), block(1024);
  for (int j = 2; j <= c.steps; j++) {
    if (halo) halo_exchange(halo, z, stop, nullptr, true);
    launch_spmv(m, z, w, nullptr, stop);
    if (j == c.steps && l1rz)
      hipLaunchKernelGGL(poly_step_k<1>, grid, block, 0, g.stream, n, r, (const double*)w, dinv, d, z, c.a[j], c.b[j], l1rz, stop);
    else
      hipLaunchKernelGGL(poly_step_k<0>, grid, block, 0, g.stream, n, r, (const double*)w, dinv, d, z, c.a[j], c.b[j], (double*)nullptr,
          stop);
  }
  HIP_CHECK(hipGetLastError());
}

// step 1 from the guess in z, behind w = A z; l1rz != NULL: with the level-1 values of r.z
static void mgp_first(uint32_t n, const double* r, const double* w, const double* dinv, double* d, double* z, double c1, double* l1rz,
    const int* stop)
{
  if (!n) return;
  const dim3 grid(vec_stream_grid(n)), block(1024);
  if (l1rz) hipLaunchKernelGGL(mgp_first_k<1>, grid, block, 0, g.stream, n, r, w, dinv, d, z, c1, l1rz, stop);
  else hipLaunchKernelGGL(mgp_first_k<0>, grid, block, 0, g.stream, n, r, w, dinv, d, z, c1, (double*)nullptr, stop);
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
// lmax where the caller gave none: the largest of g's row bounds.  where: "" or "level l: ", as the message names the matrix
static double poly_lmax_bound(const std::vector<double>& g, const char* fn, const char* where)
{
  double lmax = 0.0;
  for (double v : g) {
    if (!(v > 0.0 && v < INFINITY)) { // a NaN would otherwise drop out of the maximum
      lmax = v;
      break;
    }
    if (v > lmax) lmax = v;
  }
  if (!(lmax > 0.0 && lmax < INFINITY))
    SB_FATAL("%s: %slmax = %g: the bound on the largest eigenvalue of D^-1 A (the largest absolute row sum of D^-1/2 A D^-1/2) is "
             "not finite and positive; pass lmax", fn, where, lmax);
  return lmax;
}

// grid of poly_step_k, poly_update_r_k and mgp_first_k over n rows: vec_stream_grid
void sb_pcg_poly_step_launch(uint32_t n, uint32_t out[3])
{
  need_init();
  out[0] = vec_stream_grid(n), out[1] = 1024u, out[2] = (uint32_t)g.prop.multiProcessorCount;
}
void sb_pcg_mg_poly_first_launch(uint32_t n, uint32_t out[3]) { sb_pcg_poly_step_launch(n, out); }

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
