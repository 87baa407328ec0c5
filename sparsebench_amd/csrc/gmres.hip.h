// gmres.hip.h -- gfx950 (wave64) kernels of restarted GMRES(m) with classical Gram-Schmidt + one reorthogonalisation (CGS2).
//
// The contract is DESIGN 4.8: every dot is the canonical tree dot of kernels.hip.h (level 0: xor butterfly per 64 elements,
// level 1: ((q0 + q1) + q2) + q3 per 256, level 2: reduce_final_1024), every product is rounded before its add or subtract
// (-ffp-contract=off), projections are subtracted in ascending basis index.  The hot path is the Krylov basis V (m + 1 vectors,
// vector i at V + i * ldv): one Arnoldi step at cycle position j reads j + 1 of them three times.  Two kernels do that work:
//   gm_multidot_k    a wave owns whole aligned 256-row groups (as dot_l1_k does), keeps the group's w in registers and walks
//                    i = 0 .. nvec-1 with MD_UNROLL vectors' loads in flight: level-1 values of all nvec dots from ONE read of w;
//   gm_multiupdate_k w (-/+)= c[i] * V[i], ascending i, one read of each V[i], one read and one write of w, and on the way out
//                    the level-1 values of the NEXT pass's dots against the updated w (EPI 2) or of w . w (EPI 1).
// gm_finish_dots_k finishes dot i in workgroup i (levels 1-2 in one workgroup, never inside a consumer: at 128^3 that would be
// 31 x 64 KB per workgroup).  No kernel waits on another workgroup; every kernel of the loop returns at once when the control
// block's stop flag is set.
#pragma once
#include "kernels.hip.h"

namespace sbk {

// Control block of the GMRES loop (HBM; written by sb_gmres_start, read back by sb_gmres_finish).  The small dense state of a
// cycle follows it in the same allocation (GmView).
struct GmScalars {
  double normr; // the residual norm the next loop test sees: the estimate |g[j+1]| inside a cycle, sqrt(r.r) at its start
  double eps;
  double hn;    // ||w|| of the last step (the op list's divide-by-scalar reads it)
  double rr;    // the last explicit r.r
  int stop;     // 1: the loop `k < itermax && normr > eps` has exited; every kernel of the loop returns
  int k;        // the iteration counter (starts at 1; returned)
  int j;        // columns of the open cycle (0: no cycle open)
  int itermax;
  int n_res;    // entries of res_hist
  int n_rr;     // entries of rr_hist
  int hist_cap;
  int cycles;   // cycles closed
  int steps;    // Arnoldi steps run
};
struct GmView { // device pointers into the state block; m = restart length, H column j at H + j * (m + 1)
  GmScalars* S;
  double *H, *cs, *sn, *g, *y, *h1, *h2, *nh1, *nh2, *hcol, *res_hist, *rr_hist;
  int m;
};

// two consecutive elements e, e + 1 of a vector of n (e even): missing ones are +0.0
__device__ __forceinline__ double2 gm_load2(const double* __restrict__ v, uint32_t e, uint32_t n)
{
  double2 r = { 0.0, 0.0 };
  if (e + 1u < n) r = *reinterpret_cast<const double2*>(v + e);
  else if (e < n) r.x = v[e];
  return r;
}
__device__ __forceinline__ void gm_store2(double* v, uint32_t e, uint32_t n, const double2& r)
{
  if (e + 1u < n) *reinterpret_cast<double2*>(v + e) = r;
  else if (e < n) v[e] = r.x;
}
// level-1 value of a 256-group from the two spans' per-lane sums (dot_l1_k's arithmetic)
__device__ __forceinline__ double gm_level1(double s0, double s1)
{
  const double t0 = butterfly32(s0), t1 = butterfly32(s1);
  const double q0 = lane_value<0>(t0), q1 = lane_value<32>(t0), q2 = lane_value<0>(t1), q3 = lane_value<32>(t1);
  return ((q0 + q1) + q2) + q3;
}
// (a missing second element contributes 0.0 * 0.0 = +0.0: the `a * b + 0.0` of dot_l1_k's odd tail)
__device__ __forceinline__ double gm_pair(const double2& a, const double2& b) { return a.x * b.x + a.y * b.y; }

constexpr int MD_UNROLL = 4; // basis vectors whose loads a wave keeps in flight together (4 x 2 KiB per wave)

// the level-1 values of dot(V[i], w), i = 0 .. nvec-1, for one 256-group whose w the wave holds: l1[i * nGroups + gI]
__device__ __forceinline__ void gm_group_dots(const double* __restrict__ V, size_t ldv, int nvec, uint32_t n, uint32_t e0,
    const double2& w0, const double2& w1, double* __restrict__ l1, uint32_t nGroups, uint32_t gI, uint32_t lane)
{
  int i = 0;
  for (; i + MD_UNROLL <= nvec; i += MD_UNROLL) {
    double2 a[MD_UNROLL], b[MD_UNROLL];
#pragma unroll
    for (int u = 0; u < MD_UNROLL; u++) {
      const double* v = V + (size_t)(i + u) * ldv;
      a[u] = gm_load2(v, e0, n), b[u] = gm_load2(v, e0 + 128u, n);
    }
#pragma unroll
    for (int u = 0; u < MD_UNROLL; u++) {
      const double val = gm_level1(gm_pair(a[u], w0), gm_pair(b[u], w1));
      if (lane == 0) l1[(size_t)(i + u) * nGroups + gI] = val;
    }
  }
  for (; i < nvec; i++) {
    const double* v  = V + (size_t)i * ldv;
    const double2 a  = gm_load2(v, e0, n), b = gm_load2(v, e0 + 128u, n);
    const double val = gm_level1(gm_pair(a, w0), gm_pair(b, w1));
    if (lane == 0) l1[(size_t)i * nGroups + gI] = val;
  }
}

__global__ __launch_bounds__(256) void gm_multidot_k(uint32_t n, int nvec, const double* __restrict__ V, size_t ldv,
    const double* __restrict__ w, double* __restrict__ l1, const int* __restrict__ stop)
{
  const uint32_t lane    = threadIdx.x & 63u;
  const uint32_t nGroups = (n + 255u) >> 8;
  const uint32_t nWaves  = gridDim.x * (blockDim.x >> 6);
  if (stop && *stop) return;
  for (uint32_t gI = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); gI < nGroups; gI += nWaves) {
    const uint32_t e0 = gI * 256u + lane * 2u;
    const double2 w0 = gm_load2(w, e0, n), w1 = gm_load2(w, e0 + 128u, n);
    gm_group_dots(V, ldv, nvec, n, e0, w0, w1, l1, nGroups, gI, lane);
  }
}

// workgroup i finishes dot i: out[i] = levels 1-2 of its values (l1 != 0: nGroups level-1 values at q + i * qStride; 0: level-0
// partials), nout[i] = -out[i] (the op list's waxpby-shaped projections read it), sum[i] = add[i] + out[i] (pass 2: H's column)
__global__ __launch_bounds__(1024) void gm_finish_dots_k(uint32_t nGroups, const double* __restrict__ q, size_t qStride, int l1,
    double* __restrict__ out, double* __restrict__ nout, const double* __restrict__ add, double* __restrict__ sum,
    const int* __restrict__ stop)
{
  __shared__ double lds16[16];
  if (stop && *stop) return;
  const uint32_t i   = blockIdx.x;
  const double total = reduce_final_1024(nGroups, q + (size_t)i * qStride, lds16, l1);
  if (threadIdx.x == 0) {
    out[i] = total;
    if (nout) nout[i] = -total;
    if (sum) sum[i] = add[i] + total;
  }
}

// w[e] = (..((w[e] -/+ c[0] * V[0][e]) -/+ c[1] * V[1][e]) ..), ascending i; ADD = false subtracts (the projections), true adds
// (the x update of a cycle close).  EPI 0: nothing more; 1: level-1 values of w . w into l1[gI]; 2: level-1 values of
// dot(V[i], w) against the UPDATED w into l1[i * nGroups + gI] -- the group's V tile is read a second time, 2 KiB per vector
// that this wave fetched a moment ago (DESIGN 4.8 says where that read is served from).
template <bool ADD, int EPI>
__global__ __launch_bounds__(256) void gm_multiupdate_k(uint32_t n, int nvec, const double* __restrict__ V, size_t ldv,
    const double* __restrict__ c, double* w, double* __restrict__ l1, const int* __restrict__ stop)
{
  const uint32_t lane    = threadIdx.x & 63u;
  const uint32_t nGroups = (n + 255u) >> 8;
  const uint32_t nWaves  = gridDim.x * (blockDim.x >> 6);
  if (stop && *stop) return;
  for (uint32_t gI = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); gI < nGroups; gI += nWaves) {
    const uint32_t e0 = gI * 256u + lane * 2u, e1 = e0 + 128u;
    double2 w0 = gm_load2(w, e0, n), w1 = gm_load2(w, e1, n);
    auto apply = [&](double ci, const double2& a, const double2& b) {
      if (ADD) {
        w0.x = w0.x + ci * a.x, w0.y = w0.y + ci * a.y;
        w1.x = w1.x + ci * b.x, w1.y = w1.y + ci * b.y;
      } else {
        w0.x = w0.x - ci * a.x, w0.y = w0.y - ci * a.y;
        w1.x = w1.x - ci * b.x, w1.y = w1.y - ci * b.y;
      }
    };
    int i = 0;
    for (; i + MD_UNROLL <= nvec; i += MD_UNROLL) {
      double2 a[MD_UNROLL], b[MD_UNROLL];
      double ci[MD_UNROLL];
#pragma unroll
      for (int u = 0; u < MD_UNROLL; u++) {
        const double* v = V + (size_t)(i + u) * ldv;
        a[u] = gm_load2(v, e0, n), b[u] = gm_load2(v, e1, n), ci[u] = c[i + u];
      }
#pragma unroll
      for (int u = 0; u < MD_UNROLL; u++) apply(ci[u], a[u], b[u]);
    }
    for (; i < nvec; i++) {
      const double* v = V + (size_t)i * ldv;
      apply(c[i], gm_load2(v, e0, n), gm_load2(v, e1, n));
    }
    gm_store2(w, e0, n, w0), gm_store2(w, e1, n, w1);
    if (EPI == 1) {
      // (elements behind n were loaded as +0.0 and stay +0.0 or -0.0 * ... : force them to +0.0 so that they add nothing)
      if (e0 >= n) w0.x = 0.0;
      if (e0 + 1u >= n) w0.y = 0.0;
      if (e1 >= n) w1.x = 0.0;
      if (e1 + 1u >= n) w1.y = 0.0;
      const double val = gm_level1(gm_pair(w0, w0), gm_pair(w1, w1));
      if (lane == 0) l1[gI] = val;
    } else if (EPI == 2) {
      if (e0 >= n) w0.x = 0.0;
      if (e0 + 1u >= n) w0.y = 0.0;
      if (e1 >= n) w1.x = 0.0;
      if (e1 + 1u >= n) w1.y = 0.0;
      gm_group_dots(V, ldv, nvec, n, e0, w0, w1, l1, nGroups, gI, lane);
    }
  }
}

// The divide loop of the six scale / step kernels: out = a / dv over the caller's rows first, first + stride, ..., and on the way
// out the first part of M^-1 out (pre_first, kernels.hip.h) for the vector the preconditioner is applied to next:
//   MODE -1  nothing rides (dinv, d, z unused)
//   MODE 0   a diagonal:                z = out o dinv            (all of M^-1; d is not touched)
//   MODE 1   a Chebyshev-smoothed plan: d = z = (out o dinv) * c1 (d is level 0's cheb.d; precond_cycle then runs with firstDone)
// blockDim / gridDim are read and every early return is taken in the kernel.
template <int MODE>
__device__ __forceinline__ void gm_divide_rows(uint32_t first, uint32_t stride, uint32_t n, const double* __restrict__ a, double dv,
    double* __restrict__ out, const double* __restrict__ dinv, double* __restrict__ d, double* __restrict__ z, double c1)
{
  for (uint32_t e = first; e < n; e += stride) {
    const double v = a[e] / dv;
    out[e]         = v;
    if (MODE >= 0) {
      const double f = pre_first<(MODE > 0)>(v, dinv[e], c1);
      if (MODE > 0) d[e] = f;
      z[e] = f;
    }
  }
}

// out = a / (*d): the normalisation of a basis vector; g0 != NULL: block 0 also records *g0 = *d (the start of a cycle:
// V[0] = r / normr, g[0] = normr)
__global__ __launch_bounds__(256) void gm_scale_k(uint32_t n, const double* __restrict__ a, const double* __restrict__ d,
    double* __restrict__ out, double* __restrict__ g0, const int* __restrict__ stop)
{
  if (stop && *stop) return;
  const double dv = *d;
  gm_divide_rows<-1>(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, n, a, dv, out, nullptr, nullptr, nullptr, 0.0);
  if (g0 && blockIdx.x == 0 && threadIdx.x == 0) *g0 = dv;
}

// prologue / cycle close: r.r from its partials; MODE 0 the prologue (k = 1, the first loop test), MODE 1 a cycle close inside
// the loop (the cycle restarts from the TRUE residual and the loop test is taken on it), MODE 2 the close sb_gmres_finish makes
// (r.r of the final x is recorded, never used to go on)
template <int MODE>
__global__ __launch_bounds__(1024) void gm_rr_k(uint32_t nGroups, const double* __restrict__ q, int l1, GmView gv,
    const int* __restrict__ stop)
{
  __shared__ double lds16[16];
  if (stop && *stop) return;
  const double rr = reduce_final_1024(nGroups, q, lds16, l1);
  if (threadIdx.x != 0) return;
  GmScalars* S = gv.S;
  const GmScalars in = *S;
  S->rr = rr;
  if (in.n_rr < in.hist_cap) gv.rr_hist[in.n_rr] = rr;
  S->n_rr = in.n_rr + 1;
  if (MODE == 0) {
    const double normr = sqrt(rr);
    S->normr = normr;
    if (0 < in.hist_cap) gv.res_hist[0] = normr;
    S->n_res = 1;
    S->k = 1, S->j = 0;
    if (!(1 < in.itermax && normr > in.eps)) S->stop = 1;
  } else {
    S->cycles = in.cycles + 1;
    S->j      = 0;
    if (MODE == 1) {
      const double normr = sqrt(rr);
      S->normr = normr;
      if (!(in.k < in.itermax && normr > in.eps)) S->stop = 1;
    }
  }
}

// The scalar step of one Arnoldi step at cycle position j (in exactly that order): hn = sqrt(w . w), the earlier
// Givens rotations on column j, the new rotation, g, the estimate, res_hist, the loop test.  Taken by thread 0 of workgroup 0.
__device__ __forceinline__ void gm_scalar_step(const GmView& gv, const GmScalars& in, int j, double hn)
{
  GmScalars* S = gv.S;
  double* Hj   = gv.H + (size_t)j * (gv.m + 1);
  for (int i = 0; i <= j; i++) Hj[i] = gv.hcol[i];
  for (int i = 0; i < j; i++) {
    const double ci = gv.cs[i], si = gv.sn[i], a = Hj[i], b = Hj[i + 1];
    const double t = ci * a + si * b;
    Hj[i + 1]      = ci * b - si * a;
    Hj[i]          = t;
  }
  const double hjj = Hj[j];
  const double d   = sqrt(hjj * hjj + hn * hn);
  const double c = hjj / d, s = hn / d;
  gv.cs[j] = c, gv.sn[j] = s, Hj[j] = d;
  const double gj = gv.g[j];
  const double gn = -(s * gj);
  gv.g[j + 1] = gn;
  gv.g[j]     = c * gj;
  const double normr = fabs(gn);
  S->normr = normr, S->hn = hn;
  if (in.k < in.hist_cap) gv.res_hist[in.k] = normr;
  S->n_res = in.k + 1;
  const int k = in.k + 1;
  S->k = k, S->j = j + 1, S->steps = in.steps + 1;
  if (!(k < in.itermax && normr > in.eps)) S->stop = 1; // the cycle stays open: sb_gmres_finish closes it from S->j
}

// SCALE = true (the fused loop): EVERY workgroup reduces the level-1 values of w . w itself in the canonical order (identical
// bits everywhere, as cg_update_r_k<1> does for alpha) and writes its share of V[j+1] = w / hn; workgroup 0 also takes the
// scalar step.  Nobody waits for anybody.  (A late workgroup may already see the stop flag the step raises: V[j+1] is then
// incomplete and never read -- a cycle closes over V[0 .. j].)  SCALE = false (the op list): one workgroup, the step only;
// l1 = 0: q holds level-0 partials.
template <bool SCALE>
__global__ __launch_bounds__(1024) void gm_step_k(uint32_t n, uint32_t nGroups, const double* __restrict__ q, int l1, GmView gv,
    int j, const double* __restrict__ w, double* __restrict__ vnext)
{
  __shared__ double lds16[16];
  const bool recorder = blockIdx.x == 0 && threadIdx.x == 0;
  GmScalars in;
  if (recorder) in = *gv.S;
  const int stopped = gv.S->stop;
  const double ww   = reduce_final_1024(nGroups, q, lds16, l1);
  if (stopped) return;
  const double hn = sqrt(ww);
  if (recorder) gm_scalar_step(gv, in, j, hn);
  if (SCALE) gm_divide_rows<-1>(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, n, w, hn, vnext, nullptr, nullptr, nullptr, 0.0);
}

// back substitution of a cycle close over its nvec columns (one thread):
//   y[i] = (..((g[i] - H[i][i+1] y[i+1]) - H[i][i+2] y[i+2]) .. - H[i][nvec-1] y[nvec-1]) / H[i][i],  i = nvec-1 .. 0
__global__ __launch_bounds__(64) void gm_backsolve_k(GmView gv, int nvec, const int* __restrict__ stop)
{
  if (stop && *stop) return;
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const size_t ld = (size_t)gv.m + 1;
  for (int i = nvec - 1; i >= 0; i--) {
    double t = gv.g[i];
    for (int l = i + 1; l < nvec; l++) t = t - gv.H[(size_t)l * ld + i] * gv.y[l];
    gv.y[i] = t / gv.H[(size_t)i * ld + i];
  }
}

// =============================================================================
// Right-preconditioned GMRES: the three kernels that PRODUCE a vector the preconditioner is applied to next also
// write the first part of M^-1 of it (pre_first<MODE>, kernels.hip.h), as bicg_plan_update_p_k<1> does for BiCGStab and
// poly_update_r_k for PCG.  Each stands in for an unpreconditioned kernel, whose bits V, x, H, g and the estimate are.  The scale
// and step kernels share their loop with it (gm_divide_rows); the multi-update is a twin, below.
// =============================================================================
// gm_scale_k with the first part of M^-1 out: out = a / (*d0), g0
template <int MODE>
__global__ __launch_bounds__(256) void gm_pre_scale_k(uint32_t n, const double* __restrict__ a, const double* __restrict__ d0,
    double* __restrict__ out, double* __restrict__ g0, const double* __restrict__ dinv, double* __restrict__ d, double* __restrict__ z,
    double c1, const int* __restrict__ stop)
{
  if (stop && *stop) return;
  const double dv = *d0;
  gm_divide_rows<MODE>(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, n, a, dv, out, dinv, d, z, c1);
  if (g0 && blockIdx.x == 0 && threadIdx.x == 0) *g0 = dv;
}

// gm_step_k<true> with the first part of M^-1 V[j+1]: the scalar step, V[j+1] = w / hn
template <int MODE>
__global__ __launch_bounds__(1024) void gm_pre_step_k(uint32_t n, uint32_t nGroups, const double* __restrict__ q, int l1, GmView gv, int j,
    const double* __restrict__ w, double* __restrict__ vnext, const double* __restrict__ dinv, double* __restrict__ d,
    double* __restrict__ z, double c1)
{
  __shared__ double lds16[16];
  const bool recorder = blockIdx.x == 0 && threadIdx.x == 0;
  GmScalars in;
  if (recorder) in = *gv.S;
  const int stopped = gv.S->stop;
  const double ww   = reduce_final_1024(nGroups, q, lds16, l1);
  if (stopped) return;
  const double hn = sqrt(ww);
  if (recorder) gm_scalar_step(gv, in, j, hn);
  gm_divide_rows<MODE>(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, n, w, hn, vnext, dinv, d, z, c1);
}

// gm_multiupdate_k<true, 0>'s twin (the x update of a cycle close): w += c[i] * V[i], ascending i, and the first part of M^-1 w.
// Its group loop (from `int i = 0` to the tail loop) is the twin's statement for statement, to be changed with it.  Tried as one
// __forceinline__ template -- the loop over (V, ldv, nvec, c, n, e0, e1) with w0 / w1 by reference, with and without __restrict__
// on V and c, and with the apply lambda left in the kernel and handed in as a functor -- every wording gave the same result:
// gm_multiupdate_k<false, 0>, <false, 1>, <true, 0> and both gm_pre_multiupdate_k lose two scalar instructions (the address
// arithmetic of the unrolled loads is scheduled differently: vector-equal only), and gm_multiupdate_k<false, 2> goes from 71 to 69
// SGPRs and from 55 to 56 VGPRs.  DESIGN 4.6 keeps a sharing only where every symbol stays identical.
template <int MODE>
__global__ __launch_bounds__(256) void gm_pre_multiupdate_k(uint32_t n, int nvec, const double* __restrict__ V, size_t ldv,
    const double* __restrict__ c, double* w, const double* __restrict__ dinv, double* __restrict__ d, double* __restrict__ z, double c1,
    const int* __restrict__ stop)
{
  const uint32_t lane    = threadIdx.x & 63u;
  const uint32_t nGroups = (n + 255u) >> 8;
  const uint32_t nWaves  = gridDim.x * (blockDim.x >> 6);
  if (stop && *stop) return;
  for (uint32_t gI = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); gI < nGroups; gI += nWaves) {
    const uint32_t e0 = gI * 256u + lane * 2u, e1 = e0 + 128u;
    double2 w0 = gm_load2(w, e0, n), w1 = gm_load2(w, e1, n);
    const double2 i0 = gm_load2(dinv, e0, n), i1 = gm_load2(dinv, e1, n);
    auto apply = [&](double ci, const double2& a, const double2& b) {
      w0.x = w0.x + ci * a.x, w0.y = w0.y + ci * a.y;
      w1.x = w1.x + ci * b.x, w1.y = w1.y + ci * b.y;
    };
    int i = 0;
    for (; i + MD_UNROLL <= nvec; i += MD_UNROLL) {
      double2 a[MD_UNROLL], b[MD_UNROLL];
      double ci[MD_UNROLL];
#pragma unroll
      for (int u = 0; u < MD_UNROLL; u++) {
        const double* v = V + (size_t)(i + u) * ldv;
        a[u] = gm_load2(v, e0, n), b[u] = gm_load2(v, e1, n), ci[u] = c[i + u];
      }
#pragma unroll
      for (int u = 0; u < MD_UNROLL; u++) apply(ci[u], a[u], b[u]);
    }
    for (; i < nvec; i++) {
      const double* v = V + (size_t)i * ldv;
      apply(c[i], gm_load2(v, e0, n), gm_load2(v, e1, n));
    }
    gm_store2(w, e0, n, w0), gm_store2(w, e1, n, w1);
    double2 f0, f1;
    f0.x = pre_first<MODE>(w0.x, i0.x, c1), f0.y = pre_first<MODE>(w0.y, i0.y, c1);
    f1.x = pre_first<MODE>(w1.x, i1.x, c1), f1.y = pre_first<MODE>(w1.y, i1.y, c1);
    if (MODE) gm_store2(d, e0, n, f0), gm_store2(d, e1, n, f1);
    gm_store2(z, e0, n, f0), gm_store2(z, e1, n, f1);
  }
}

// test entry (sb_debug_sqrt_div): the device's sqrt and / on caller-supplied operands
__global__ __launch_bounds__(256) void gm_sqrt_div_k(uint32_t n, const double* __restrict__ a, const double* __restrict__ b,
    double* __restrict__ sq, double* __restrict__ dv)
{
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) sq[e] = sqrt(a[e]), dv[e] = a[e] / b[e];
}

} // namespace sbk
