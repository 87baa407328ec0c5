// bicgstab.hip.h -- kernels of right-preconditioned BiCGStab with a diagonal preconditioner, and the two updates it
// runs under a preconditioner plan of PCG's in the diagonal's place.  wave64, fp64.
//
// Every operation is rounded on its own (the TU is compiled with -ffp-contract=off): alpha * v is one multiply, r - (alpha * v)
// one subtraction, and so on, in the order DESIGN 4.11 writes them.  Every dot is the canonical dot of kernels.hip.h (level 0
// butterfly32 halves of a 128-element span, level 1 ((q0 + q1) + q2) + q3 per aligned 256-row group, level 2 reduce_final_1024).
// The loop has a control block of its own (BicgScalars); CgScalars, PcgScalars and every kernel that reads them are untouched.
#pragma once
#include "kernels.hip.h"

namespace sbk {

// Control block of the BiCGStab loop (HBM; written by the host once per solve, read once at the end)
struct BicgScalars {
  double rr;       // r.r: the loop test's quantity (normr = sqrt(rr))
  double rho;      // rhat.r
  double rho_old;
  double rv;       // rhat.v: alpha = rho / rv
  double alpha;
  double ts;       // t.s
  double tt;       // t.t: omega = ts / tt
  double omega;
  double beta;     // (rho / rho_old) * (alpha / omega)
  double eps;
  int stop;      // 1: the for loop has exited; every kernel returns
  int iters;     // k of the last loop body that runs / ran
  int n_rr;      // entries written to the rr and to the rho history (always together)
  int n_rv;      // entries written to the rv history
  int n_ts;      // entries written to the ts and to the tt history (always together)
  int itermax;
  int hist_cap;  // entries per history; the five histories lie behind one another: rr, rho, rv, ts, tt
  int pad_;
};

// =============================================================================
// The streaming skeleton of the four vector kernels: pcg_update_r_k's shape with NIN input streams, NOUT output streams and
// NDOT (0, 1, 2) dots.  A wave owns whole aligned 256-row groups (two adjacent 128-element spans, lane l holds elements 2l,
// 2l + 1 of each) and strides over them by the number of waves in the grid.  The first group's loads go in flight BEFORE
// prep() reads the control block (prep returns false where the loop has stopped: the wave leaves); a wave's further groups
// (n above 256 rows x the grid's waves: 2.1 M rows on 256 CUs) are loaded and processed in turn, no register is carried round
// the loop.  elem(w, o, ta, tb) is the
// arithmetic of ONE row: w its NIN inputs, o its NOUT outputs, ta and tb its products for the two dots.  The skeleton moves
// rows two at a time (16-byte loads and stores) and adds their products as x + y; the single last row of an odd n adds
// + 0.0.  The level-1 values are formed in registers from butterfly32 partials as ((q0 + q1) + q2) + q3 and handed to
// emit(group, va, vb) on lane 0.  A guarded loop takes the partial last group.  An output may be an input's storage: a row
// is read before it is written and no other thread touches it.
// =============================================================================
template <int NIN, int NOUT, int NDOT, class Prep, class Elem, class Emit>
__device__ __forceinline__ void bicg_stream(uint32_t n, const double* const (&in)[NIN], double* const (&out)[NOUT ? NOUT : 1], Prep&& prep,
    Elem&& elem, Emit&& emit)
{
  constexpr int NO       = NOUT ? NOUT : 1;
  const uint32_t lane    = threadIdx.x & 63u;
  const uint32_t nGroups = (n + 255u) >> 8;
  const uint32_t nWaves  = gridDim.x * (blockDim.x >> 6);
  uint32_t gI            = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  auto full = [&](uint32_t gg) { return gg < nGroups && gg * 256u + 256u <= n; }; // wave-uniform
  double x0[NIN], y0[NIN], x1[NIN], y1[NIN]; // rows e0, e0 + 1 of the first span, e1, e1 + 1 of the second
#pragma unroll
  for (int u = 0; u < NIN; u++) x0[u] = y0[u] = x1[u] = y1[u] = 0.0;
  auto load = [&](uint32_t gg) {
    const uint32_t e0 = gg * 256u + lane * 2u, e1 = e0 + 128u;
#pragma unroll
    for (int u = 0; u < NIN; u++) {
      const double2 a = *reinterpret_cast<const double2*>(in[u] + e0);
      const double2 b = *reinterpret_cast<const double2*>(in[u] + e1);
      x0[u] = a.x, y0[u] = a.y, x1[u] = b.x, y1[u] = b.y;
    }
  };
  // two adjacent rows at e: outputs stored, dot terms returned
  auto two = [&](uint32_t e, const double(&wx)[NIN], const double(&wy)[NIN], double& sa, double& sb) {
    double ox[NO], oy[NO], tax = 0.0, tay = 0.0, tbx = 0.0, tby = 0.0;
    elem(wx, ox, tax, tbx);
    elem(wy, oy, tay, tby);
#pragma unroll
    for (int o = 0; o < NOUT; o++) {
      double2 t;
      t.x = ox[o], t.y = oy[o];
      *reinterpret_cast<double2*>(out[o] + e) = t;
    }
    sa = tax + tay, sb = tbx + tby;
  };
  bool have = full(gI);
  if (have) load(gI);
  if (!prep()) return;
  auto combine = [&](double t0, double t1) { // halves of t0: q0, q1; of t1: q2, q3
    const double q0 = lane_value<0>(t0), q1 = lane_value<32>(t0), q2 = lane_value<0>(t1), q3 = lane_value<32>(t1);
    return ((q0 + q1) + q2) + q3;
  };
  auto group = [&](uint32_t gg) { // one full group from the registers
    const uint32_t e0 = gg * 256u + lane * 2u, e1 = e0 + 128u;
    double a0 = 0.0, b0 = 0.0, a1 = 0.0, b1 = 0.0;
    two(e0, x0, y0, a0, b0);
    two(e1, x1, y1, a1, b1);
    if constexpr (NDOT > 0) {
      const double va = combine(butterfly32(a0), butterfly32(a1));
      double vb       = 0.0;
      if constexpr (NDOT > 1) vb = combine(butterfly32(b0), butterfly32(b1));
      if (lane == 0) emit(gg, va, vb);
    }
  };
  if (have) { // the group whose loads went out beside the control block, then the wave's further full groups
    group(gI);
    for (gI += nWaves; full(gI); gI += nWaves) {
      load(gI);
      group(gI);
    }
  }
  for (; gI < nGroups; gI += nWaves) { // the last, partial group
    double ta[2] = { 0.0, 0.0 }, tb[2] = { 0.0, 0.0 };
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const uint32_t e = gI * 256u + (uint32_t)h * 128u + lane * 2u;
      double sa = 0.0, sb = 0.0;
      if (e + 1 < n) {
        double wx[NIN], wy[NIN];
#pragma unroll
        for (int u = 0; u < NIN; u++) {
          const double2 a = *reinterpret_cast<const double2*>(in[u] + e);
          wx[u] = a.x, wy[u] = a.y;
        }
        two(e, wx, wy, sa, sb);
      } else if (e < n) {
        double w[NIN], o[NO], pa = 0.0, pb = 0.0;
#pragma unroll
        for (int u = 0; u < NIN; u++) w[u] = in[u][e];
        elem(w, o, pa, pb);
#pragma unroll
        for (int q = 0; q < NOUT; q++) out[q][e] = o[q];
        sa = pa + 0.0, sb = pb + 0.0;
      }
      if constexpr (NDOT > 0) ta[h] = butterfly32(sa);
      if constexpr (NDOT > 1) tb[h] = butterfly32(sb);
    }
    if constexpr (NDOT > 0) {
      const double va = combine(ta[0], ta[1]);
      double vb       = 0.0;
      if constexpr (NDOT > 1) vb = combine(tb[0], tb[1]);
      if (lane == 0) emit(gI, va, vb);
    }
  }
}

// The two updates that make a vector M^-1 is applied to next, each written once for the three things M^-1 can be:
//   MODE -1  the sweeps of a plan: p (s) alone; the plan's cycle makes ph (sh) from zero.  dinv, d, ph unused
//   MODE 0   a diagonal: ph = p o dinv, all of M^-1
//   MODE 1   a Chebyshev-smoothed plan: level 0's step 1 rides here, as it rides in poly_update_r_k for PCG: d = (p o dinv) * c1
//            and ph = d (pre_first, kernels.hip.h); d is level 0's cheb.d
// p = r + beta * (p - omega * v).  Three streams in (r, p, v) and with a MODE a fourth (dinv); one out, and ph, and d.  The first
// body runs it literally on p = v = 0, beta = omega = 0.0.
template <int MODE>
__device__ __forceinline__ void bicg_update_p_rows(uint32_t n, const double* __restrict__ r, double* p, const double* __restrict__ v,
    const double* __restrict__ dinv, double* __restrict__ d, double* __restrict__ ph, double c1, const BicgScalars* S)
{
  constexpr int NIN = MODE < 0 ? 3 : 4, NOUT = MODE < 0 ? 1 : 2 + MODE;
  const double* in[NIN];
  double* out[NOUT];
  in[0] = r, in[1] = p, in[2] = v, out[0] = p;
  if constexpr (MODE >= 0) in[3] = dinv, out[NOUT - 1] = ph;
  if constexpr (MODE > 0) out[1] = d;
  const double* const(&cin)[NIN] = in;
  double* const(&cout)[NOUT]     = out;
  double beta = 0.0, omega = 0.0;
  bicg_stream<NIN, NOUT, 0>(
      n, cin, cout,
      [&] {
        if (S->stop) return false;
        beta = S->beta, omega = S->omega;
        return true;
      },
      [&](const double(&w)[NIN], double(&o)[NOUT], double&, double&) {
        const double t1 = omega * w[2];
        const double t2 = w[1] - t1;
        const double t3 = beta * t2;
        o[0]            = w[0] + t3;
        if constexpr (MODE >= 0) {
          o[NOUT - 1] = pre_first<(MODE > 0)>(o[0], w[NIN - 1], c1);
          if constexpr (MODE > 0) o[1] = o[NOUT - 1];
        }
      },
      [&](uint32_t, double, double) {});
}
// s = r - alpha * v; s may be r's storage (the loop's is).  Two streams in (r, v) and with a MODE a third (dinv)
template <int MODE>
__device__ __forceinline__ void bicg_update_s_rows(uint32_t n, const double* r, const double* __restrict__ v, const double* __restrict__ dinv,
    double* s, double* __restrict__ d, double* __restrict__ sh, double c1, const BicgScalars* S)
{
  constexpr int NIN = MODE < 0 ? 2 : 3, NOUT = MODE < 0 ? 1 : 2 + MODE;
  const double* in[NIN];
  double* out[NOUT];
  in[0] = r, in[1] = v, out[0] = s;
  if constexpr (MODE >= 0) in[2] = dinv, out[NOUT - 1] = sh;
  if constexpr (MODE > 0) out[1] = d;
  const double* const(&cin)[NIN] = in;
  double* const(&cout)[NOUT]     = out;
  double alpha = 0.0;
  bicg_stream<NIN, NOUT, 0>(
      n, cin, cout,
      [&] {
        if (S->stop) return false;
        alpha = S->alpha;
        return true;
      },
      [&](const double(&w)[NIN], double(&o)[NOUT], double&, double&) {
        const double t1 = alpha * w[1];
        o[0]            = w[0] - t1;
        if constexpr (MODE >= 0) {
          o[NOUT - 1] = pre_first<(MODE > 0)>(o[0], w[NIN - 1], c1);
          if constexpr (MODE > 0) o[1] = o[NOUT - 1];
        }
      },
      [&](uint32_t, double, double) {});
}

// the diagonal's two kernels
__global__ __launch_bounds__(1024) void bicg_update_p_k(uint32_t n, const double* __restrict__ r, double* p, const double* __restrict__ v,
    const double* __restrict__ dinv, double* __restrict__ ph, const BicgScalars* S)
{
  bicg_update_p_rows<0>(n, r, p, v, dinv, nullptr, ph, 0.0, S);
}
__global__ __launch_bounds__(1024) void bicg_update_s_k(uint32_t n, const double* r, const double* __restrict__ v,
    const double* __restrict__ dinv, double* s, double* __restrict__ sh, const BicgScalars* S)
{
  bicg_update_s_rows<0>(n, r, v, dinv, s, nullptr, sh, 0.0, S);
}
// a plan's two: CHEB 0 the sweeps, CHEB 1 the polynomial
template <int CHEB>
__global__ __launch_bounds__(1024) void bicg_plan_update_p_k(uint32_t n, const double* __restrict__ r, double* p, const double* __restrict__ v,
    const double* __restrict__ dinv, double* __restrict__ d, double* __restrict__ ph, double c1, const BicgScalars* S)
{
  bicg_update_p_rows<CHEB ? 1 : -1>(n, r, p, v, dinv, d, ph, c1, S);
}
template <int CHEB>
__global__ __launch_bounds__(1024) void bicg_plan_update_s_k(uint32_t n, const double* r, const double* __restrict__ v,
    const double* __restrict__ dinv, double* s, double* __restrict__ d, double* __restrict__ sh, double c1, const BicgScalars* S)
{
  bicg_update_s_rows<CHEB ? 1 : -1>(n, r, v, dinv, s, d, sh, c1, S);
}

// the level-1 values of a.b and of a.a from one pass over a and b: t.s and t.t, and in the prologue r.rhat and r.r.  (The
// single dot rhat.v is dot_l1_k of kernels.hip.h, unchanged.)  stop: NULL, or the loop's stop flag.
__global__ __launch_bounds__(1024) void bicg_dot2_k(uint32_t n, const double* __restrict__ a, const double* __restrict__ b,
    double* __restrict__ l1ab, double* __restrict__ l1aa, const int* __restrict__ stop)
{
  const double* const in[2] = { a, b };
  double* const out[1]      = { nullptr };
  bicg_stream<2, 0, 2>(
      n, in, out, [&] { return !(stop && *stop); },
      [&](const double(&w)[2], double(&)[1], double& ta, double& tb) { ta = w[0] * w[1], tb = w[0] * w[0]; },
      [&](uint32_t gI, double va, double vb) { l1ab[gI] = va, l1aa[gI] = vb; });
}

// x = (x + alpha * ph) + omega * sh ;  r = s - omega * t ;  the level-1 values of rhat.r and of r.r.  Six streams in
// (x, ph, sh, s, t, rhat), two out; r may be s's storage (the loop's is).
__global__ __launch_bounds__(1024) void bicg_update_xr_k(uint32_t n, double* x, const double* __restrict__ ph, const double* __restrict__ sh,
    const double* s, const double* __restrict__ t, const double* __restrict__ rhat, double* r, const BicgScalars* S,
    double* __restrict__ l1rho, double* __restrict__ l1rr)
{
  const double* const in[6] = { x, ph, sh, s, t, rhat };
  double* const out[2]      = { x, r };
  double alpha = 0.0, omega = 0.0;
  bicg_stream<6, 2, 2>(
      n, in, out,
      [&] {
        if (S->stop) return false;
        alpha = S->alpha, omega = S->omega;
        return true;
      },
      [&](const double(&w)[6], double(&o)[2], double& ta, double& tb) {
        const double a1 = alpha * w[1];
        const double x1 = w[0] + a1;
        const double a2 = omega * w[2];
        o[0]            = x1 + a2;
        const double o1 = omega * w[4];
        o[1]            = w[3] - o1;
        ta = w[5] * o[1], tb = o[1] * o[1];
      },
      [&](uint32_t gI, double va, double vb) { l1rho[gI] = va, l1rr[gI] = vb; });
}

// The scalar steps, ONE workgroup of 1024 threads, m level-1 values per dot in.
//   MODE 0  prologue: rho = rhat.r from qa, rr from qb; records rr[0], rho[0]; the loop test for k = 1
//   MODE 1  alpha step: rv from qa, alpha = rho / rv; records rv
//   MODE 2  omega step: ts from qa, tt from qb, omega = ts / tt; records both
//   MODE 3  beta step: rho_old = rho, rho from qa, rr from qb, beta = (rho / rho_old) * (alpha / omega); records rr and rho;
//           the loop test for the next k on the new rr: it passes, or the stop flag goes up
// The reductions run before the branch on the control block (every thread reaches reduce_final_1024's barrier).
template <int MODE>
__global__ __launch_bounds__(1024) void bicg_scalar_k(uint32_t m, const double* __restrict__ qa, const double* __restrict__ qb, BicgScalars* S,
    double* __restrict__ hist)
{
  __shared__ double ldsA[16], ldsB[16];
  const BicgScalars in = *S;
  const double ta      = reduce_final_1024(m, qa, ldsA, 1);
  const double tb      = MODE == 1 ? 0.0 : reduce_final_1024(m, qb, ldsB, 1);
  if (in.stop || threadIdx.x != 0) return;
  const size_t cap = (size_t)in.hist_cap;
  if (MODE == 0 || MODE == 3) {
    if (MODE == 3) {
      S->rho_old      = in.rho;
      const double q1 = ta / in.rho;
      const double q2 = in.alpha / in.omega;
      S->beta         = q1 * q2;
    }
    S->rho = ta, S->rr = tb;
    if (in.n_rr < in.hist_cap) hist[in.n_rr] = tb, hist[cap + (size_t)in.n_rr] = ta;
    S->n_rr       = in.n_rr + 1;
    const int nxt = MODE == 0 ? 1 : in.iters + 1;
    if (nxt < in.itermax && sqrt(tb) > in.eps) S->iters = nxt;
    else S->stop = 1;
  } else if (MODE == 1) {
    S->rv    = ta;
    S->alpha = in.rho / ta;
    if (in.n_rv < in.hist_cap) hist[2 * cap + (size_t)in.n_rv] = ta;
    S->n_rv = in.n_rv + 1;
  } else {
    S->ts = ta, S->tt = tb;
    S->omega = ta / tb;
    if (in.n_ts < in.hist_cap) hist[3 * cap + (size_t)in.n_ts] = ta, hist[4 * cap + (size_t)in.n_ts] = tb;
    S->n_ts = in.n_ts + 1;
  }
}

} // namespace sbk
