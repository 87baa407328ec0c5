// pcg.hip.h -- kernels of diagonally preconditioned CG: solveCG's loop with z = r o dinv put back.  wave64, fp64.
//
// Every operation is rounded on its own (the TU is compiled with -ffp-contract=off): z_i = r_i * dinv_i is one multiply, the
// dots r.z and r.r are the canonical dot of kernels.hip.h (level 0 butterfly32 halves of a 128-element span, level 1
// ((q0 + q1) + q2) + q3 per aligned 256-row group, level 2 reduce_final_1024).  With dinv = 1.0 everywhere z is r bit for bit,
// r.z is r.r, and the loop is sb_cg's: the identity tests hold it to that.
// The loop has a control block of its own (PcgScalars); CgScalars and every kernel that reads it are untouched.
#pragma once
#include "kernels.hip.h"

namespace sbk {

// Control block of the PCG loop (HBM; written by the host once per solve, read once at the end)
struct PcgScalars {
  double rr;        // r.r: the loop test's quantity (normr = sqrt(rr))
  double rz;        // r.z: alpha = rz / pAp, beta = rz / rz_old
  double rz_old;
  double pAp;
  double alpha;
  double beta;
  double neg_alpha;
  double eps;
  int stop;       // 1: the for loop has exited; every kernel returns
  int stop_next;  // !(normr > eps) for the normr the NEXT loop test will see
  int iters;      // k of the last loop body that runs / ran
  int n_rr;       // entries written to rr_hist and to rz_hist (always together)
  int n_pAp;
  int itermax;
  int hist_cap;
  int x_pending;  // 1: x += alpha p of the last body is still owed (applied by the next p update)
};

// the control block into registers, pinned in front of whatever follows (cg_fetch for this block)
__device__ __forceinline__ PcgScalars pcg_fetch(const PcgScalars* S)
{
  const PcgScalars in = *S;
  asm volatile("" ::"v"(in.rr), "v"(in.rz), "v"(in.eps), "v"(in.stop), "v"(in.stop_next), "v"(in.iters), "v"(in.n_rr), "v"(in.n_pAp),
      "v"(in.itermax), "v"(in.hist_cap));
  return in;
}

// =============================================================================
// The r update with z and both dots, once per body:
//   PRO 0   r = r + (-alpha) Ap ;  z = r o dinv ;  level-1 values of r.z and of r.r        (src = r, coefficient S->neg_alpha)
//   PRO 1   r = b + (-1.0) Ap   ;  z = r o dinv ;  the same two arrays: the prologue        (src = b)
// The shape is cg_update_r_k<0>'s: a wave owns whole aligned 256-row groups (two adjacent 128-element spans, lane l holds
// elements 2l, 2l + 1 of each), the first group's loads go in flight beside the control block, the group's level-1 values
// are formed in registers.  Six streams per row instead of three (r, Ap, dinv in; r, z out), two butterfly reductions per
// span.  The partial last group and an odd n take the guarded loop behind.
// sgs_update_r_k (sgs.hip.h) is this kernel without the dinv loads, the z stores and the r.z values: its twin, to be changed
// with it (as one body with a compile-time switch neither kernel keeps its code: DESIGN 4.6).
// =============================================================================
template <int PRO>
__global__ __launch_bounds__(1024) void pcg_update_r_k(uint32_t n, const double* __restrict__ Ap, const double* src, double* r,
    const double* __restrict__ dinv, double* __restrict__ z, const PcgScalars* S, double* __restrict__ l1rz,
    double* __restrict__ l1rr)
{
  const uint32_t lane    = threadIdx.x & 63u;
  const uint32_t nGroups = (n + 255u) >> 8;
  const uint32_t nWaves  = gridDim.x * (blockDim.x >> 6);
  uint32_t gI            = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  auto full = [&](uint32_t gg) { return gg < nGroups && gg * 256u + 256u <= n; }; // wave-uniform
  double2 r0 = { 0.0, 0.0 }, a0 = r0, d0 = r0, r1 = r0, a1 = r0, d1 = r0;
  auto load = [&](uint32_t gg) {
    const uint32_t e0 = gg * 256u + lane * 2u, e1 = e0 + 128u;
    r0 = *reinterpret_cast<const double2*>(src + e0), a0 = *reinterpret_cast<const double2*>(Ap + e0);
    r1 = *reinterpret_cast<const double2*>(src + e1), a1 = *reinterpret_cast<const double2*>(Ap + e1);
    d0 = *reinterpret_cast<const double2*>(dinv + e0), d1 = *reinterpret_cast<const double2*>(dinv + e1);
  };
  bool have = full(gI);
  if (have) load(gI);
  double c = -1.0;
  if (!PRO) {
    if (S->stop) return;
    c = S->neg_alpha;
  }
  auto combine = [&](double t0, double t1) { // halves of t0: q0, q1; of t1: q2, q3
    const double q0 = lane_value<0>(t0), q1 = lane_value<32>(t0), q2 = lane_value<0>(t1), q3 = lane_value<32>(t1);
    return ((q0 + q1) + q2) + q3;
  };
  while (have) {
    const uint32_t e0 = gI * 256u + lane * 2u, e1 = e0 + 128u;
    r0.x = r0.x + c * a0.x, r0.y = r0.y + c * a0.y;
    r1.x = r1.x + c * a1.x, r1.y = r1.y + c * a1.y;
    double2 z0, z1;
    z0.x = r0.x * d0.x, z0.y = r0.y * d0.y;
    z1.x = r1.x * d1.x, z1.y = r1.y * d1.y;
    *reinterpret_cast<double2*>(r + e0) = r0;
    *reinterpret_cast<double2*>(r + e1) = r1;
    *reinterpret_cast<double2*>(z + e0) = z0;
    *reinterpret_cast<double2*>(z + e1) = z1;
    const double vz = combine(butterfly32(r0.x * z0.x + r0.y * z0.y), butterfly32(r1.x * z1.x + r1.y * z1.y));
    const double vr = combine(butterfly32(r0.x * r0.x + r0.y * r0.y), butterfly32(r1.x * r1.x + r1.y * r1.y));
    if (lane == 0) l1rz[gI] = vz, l1rr[gI] = vr;
    gI += nWaves;
    have = full(gI);
    if (have) load(gI);
  }
  for (; gI < nGroups; gI += nWaves) { // the last, partial group
    double tz[2], tr[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const uint32_t e = gI * 256u + (uint32_t)h * 128u + lane * 2u;
      double sz = 0.0, sr = 0.0;
      if (e + 1 < n) {
        double2 rv       = *reinterpret_cast<const double2*>(src + e);
        const double2 av = *reinterpret_cast<const double2*>(Ap + e);
        const double2 dv = *reinterpret_cast<const double2*>(dinv + e);
        rv.x = rv.x + c * av.x;
        rv.y = rv.y + c * av.y;
        double2 zv;
        zv.x = rv.x * dv.x, zv.y = rv.y * dv.y;
        *reinterpret_cast<double2*>(r + e) = rv;
        *reinterpret_cast<double2*>(z + e) = zv;
        sz = rv.x * zv.x + rv.y * zv.y;
        sr = rv.x * rv.x + rv.y * rv.y;
      } else if (e < n) {
        const double rn = src[e] + c * Ap[e];
        const double zn = rn * dinv[e];
        r[e] = rn, z[e] = zn;
        sz = rn * zn + 0.0;
        sr = rn * rn + 0.0;
      }
      tz[h] = butterfly32(sz), tr[h] = butterfly32(sr);
    }
    const double vz = combine(tz[0], tz[1]), vr = combine(tr[0], tr[1]);
    if (lane == 0) l1rz[gI] = vz, l1rr[gI] = vr;
  }
}

// p = z + beta p (which = 1: the literal k = 1 form p = z + 0.0 z) with the "x += alpha p" the previous body left owing, the
// old p in registers: cg_update_p<0> statement for statement, z in r's place, on this loop's control block.
__global__ __launch_bounds__(1024) void pcg_update_p_k(uint32_t n, const double* __restrict__ z, double* p, double* x,
    const PcgScalars* S, int which)
{
  const uint32_t n2     = n >> 1;
  const uint32_t stride = gridDim.x * blockDim.x;
  const double2* z2     = reinterpret_cast<const double2*>(z);
  double2* p2           = reinterpret_cast<double2*>(p);
  double2* x2           = reinterpret_cast<double2*>(x);
  uint32_t i            = blockIdx.x * blockDim.x + threadIdx.x;
  const bool useX       = which == 0;
  const uint32_t last   = n2 ? n2 - 1u : 0u;
  double2 a0 = { 0.0, 0.0 }, b0 = a0, x0 = a0, a1 = a0, b1 = a0, x1 = a0;
  auto load = [&](uint32_t j, double2& a, double2& b, double2& xv) {
    a = z2[j];
    b = which == 0 ? p2[j] : a;
    if (useX) xv = x2[j];
  };
  if (n2) load(min(i, last), a0, b0, x0), load(min(i + stride, last), a1, b1, x1);
  const int stopped  = S->stop;
  const double beta  = which == 0 ? S->beta : 0.0;
  const bool owed    = useX && S->x_pending;
  const double alpha = S->alpha;
  if (stopped) return;
  auto finish = [&](uint32_t j, const double2& a, const double2& b, double2 xv) {
    if (owed) {
      xv.x = xv.x + alpha * b.x;
      xv.y = xv.y + alpha * b.y;
      x2[j] = xv;
    }
    double2 o;
    o.x = a.x + beta * b.x;
    o.y = a.y + beta * b.y;
    p2[j] = o;
  };
  for (; i < n2; i += 2u * stride) {
    const bool second = i + stride < n2;
    finish(i, a0, b0, x0);
    if (second) finish(i + stride, a1, b1, x1);
    const uint32_t nx = i + 2u * stride;
    if (nx < n2) load(nx, a0, b0, x0), load(min(nx + stride, last), a1, b1, x1);
  }
  if ((n & 1u) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double bb = which == 0 ? p[n - 1] : z[n - 1];
    if (owed) x[n - 1] = x[n - 1] + alpha * bb;
    p[n - 1] = z[n - 1] + beta * bb;
  }
}

// the owed "x += alpha p" of the LAST body that ran (nobody comes after it)
__global__ __launch_bounds__(256) void pcg_x_finalize(uint32_t n, double* x, const double* __restrict__ p, const PcgScalars* __restrict__ S)
{
  if (!S->x_pending) return;
  const double alpha    = S->alpha;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] = x[i] + alpha * p[i];
}
__global__ void pcg_clear_pending(PcgScalars* S) { S->x_pending = 0; }

// The scalar steps, ONE workgroup of 1024 threads, level-1 values in (m of them per dot).
//   MODE 0  prologue: rr, rz from both arrays, the loop test for k = 1; records rr[0], rz[0]
//   MODE 1  beta step: the loop test for the next k on the rr already held; if it passes, reduces both arrays' values into
//           rz_old = rz, rz, rr, beta = rz / rz_old, and the test the body after will see; else raises the stop flag.  The body
//           that just ran has left its x update owing either way.
//   MODE 2  alpha step: pAp from qa, alpha = rz / pAp; records pAp
// As in cg_scalar_k the control block is fetched beside the level-1 loads and the reductions run before the branch on it.
template <int MODE>
__global__ __launch_bounds__(1024) void pcg_scalar_k(uint32_t m, const double* __restrict__ qa, const double* __restrict__ qb,
    PcgScalars* S, double* __restrict__ rr_hist, double* __restrict__ rz_hist, double* __restrict__ pAp_hist)
{
  __shared__ double ldsA[16], ldsB[16];
  const PcgScalars in = pcg_fetch(S);
  const double ta     = reduce_final_1024(m, qa, ldsA, 1);                     // MODE 2: p.Ap; else r.z
  const double tb     = MODE == 2 ? 0.0 : reduce_final_1024(m, qb, ldsB, 1);   // r.r
  if (in.stop || threadIdx.x != 0) return;
  if (MODE == 0) {
    const int sn = !(sqrt(tb) > in.eps);
    S->rr = tb, S->rz = ta, S->stop_next = sn;
    if (in.n_rr < in.hist_cap) rr_hist[in.n_rr] = tb, rz_hist[in.n_rr] = ta;
    S->n_rr = in.n_rr + 1;
    if (1 < in.itermax && !sn) S->iters = 1;
    else S->stop = 1;
  } else if (MODE == 1) {
    if (in.iters + 1 < in.itermax && !in.stop_next) {
      S->rz_old    = in.rz;
      S->rz        = ta;
      S->rr        = tb;
      S->beta      = ta / in.rz;
      S->stop_next = !(sqrt(tb) > in.eps);
      S->iters     = in.iters + 1;
      if (in.n_rr < in.hist_cap) rr_hist[in.n_rr] = tb, rz_hist[in.n_rr] = ta;
      S->n_rr = in.n_rr + 1;
    } else {
      S->stop = 1;
    }
    S->x_pending = 1;
  } else {
    S->x_pending    = 0; // consumed by the p update that preceded this SpMV
    S->pAp          = ta;
    const double al = in.rz / ta;
    S->alpha        = al;
    S->neg_alpha    = -al;
    if (in.n_pAp < in.hist_cap) pAp_hist[in.n_pAp] = ta;
    S->n_pAp = in.n_pAp + 1;
  }
}

// =============================================================================
// The scalar steps on several ranks.  Each of p.Ap, r.z and r.r is the rank's own levels 1-2 value, then the
// pairwise tree over ranks; every rank continues with identical bits.  PcgScalars and pcg_scalar_k stay as they are: what the
// ranks add to the loop's state is a block of its own.
// =============================================================================
struct PcgRankSums {
  double v[2];   // the communicator's plane: the rank's sums, all-reduced in place (MODE 2: v[0] = p.Ap; else v[0] = r.z, v[1] = r.r)
  int p2p_error; // the peer-mapped plane: 1 a wait of an in-kernel all-reduce ran out here, 2 a peer has failed (CgScalars::p2p_error)
};

// pcg_scalar_k<MODE>'s step on the sums ta (p.Ap or r.z) and tb (r.r), statement for statement; one thread.  Its twin, to be
// changed with it: with the step taken out into this function pcg_scalar_k<0> and <1> do not keep their code
template <int MODE>
__device__ __forceinline__ void pcg_apply(PcgScalars* S, const PcgScalars& in, double ta, double tb, double* __restrict__ rr_hist,
    double* __restrict__ rz_hist, double* __restrict__ pAp_hist)
{
  if (MODE == 0) {
    const int sn = !(sqrt(tb) > in.eps);
    S->rr = tb, S->rz = ta, S->stop_next = sn;
    if (in.n_rr < in.hist_cap) rr_hist[in.n_rr] = tb, rz_hist[in.n_rr] = ta;
    S->n_rr = in.n_rr + 1;
    if (1 < in.itermax && !sn) S->iters = 1;
    else S->stop = 1;
  } else if (MODE == 1) {
    if (in.iters + 1 < in.itermax && !in.stop_next) {
      S->rz_old    = in.rz;
      S->rz        = ta;
      S->rr        = tb;
      S->beta      = ta / in.rz;
      S->stop_next = !(sqrt(tb) > in.eps);
      S->iters     = in.iters + 1;
      if (in.n_rr < in.hist_cap) rr_hist[in.n_rr] = tb, rz_hist[in.n_rr] = ta;
      S->n_rr = in.n_rr + 1;
    } else {
      S->stop = 1;
    }
    S->x_pending = 1;
  } else {
    S->x_pending    = 0;
    S->pAp          = ta;
    const double al = in.rz / ta;
    S->alpha        = al;
    S->neg_alpha    = -al;
    if (in.n_pAp < in.hist_cap) pAp_hist[in.n_pAp] = ta;
    S->n_pAp = in.n_pAp + 1;
  }
}

// The peer-mapped plane: local levels 1-2, the exchange over the P2PView, the step -- one launch, as cg_scalar_p2p_k is for CG.
// The alpha step carries one value.  The prologue's step and the beta step carry two: r.z travels as exchange `seq`, r.r as
// `seq + 1`, back to back, on the two slot sets alternately (the host advances the shared counter by two).  A rank stores its
// r.r only behind the barrier that ends its reads of every peer's r.z, and the next launch's first value only after every
// peer's r.r has arrived: no rank is two exchanges ahead of a peer, which is all the two slot sets need.
// A stopped loop skips the exchange on every rank; a raised error (R->p2p_error, or the halo plan's) poisons the slots.
template <int MODE>
__global__ __launch_bounds__(1024) void pcg_scalar_p2p_k(uint32_t m, const double* __restrict__ qa, const double* __restrict__ qb,
    PcgScalars* S, double* __restrict__ rr_hist, double* __restrict__ rz_hist, double* __restrict__ pAp_hist, PcgRankSums* R,
    const P2PView* __restrict__ pv, unsigned long long seq, const int* __restrict__ haloErr)
{
  __shared__ double ldsA[16], ldsB[16];
  const PcgScalars in = pcg_fetch(S);
  double ta           = reduce_final_1024(m, qa, ldsA, 1);
  double tb           = MODE == 2 ? 0.0 : reduce_final_1024(m, qb, ldsB, 1);
  if (in.stop) { // identical on every rank: all of them skip the exchange, or none -- unless one has failed
    if (__hip_atomic_load(&R->p2p_error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) || (haloErr && *haloErr)) p2p_poison_allreduce(pv);
    return;
  }
  __syncthreads(); // the LDS arrays are reused
  ta = p2p_allreduce_sum(pv, ta, seq, ldsA, &R->p2p_error);
  // (uniform: an error is raised before the barriers inside the exchange; a failed first exchange does not start the second)
  if (MODE != 2 && !__hip_atomic_load(&R->p2p_error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    tb = p2p_allreduce_sum(pv, tb, seq + 1ull, ldsB, &R->p2p_error);
  if (__hip_atomic_load(&R->p2p_error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
    if (threadIdx.x == 0) S->stop = 1;
    p2p_poison_allreduce(pv); // (and tell the others at once)
    return;
  }
  if (threadIdx.x == 0) pcg_apply<MODE>(S, in, ta, tb, rr_hist, rz_hist, pAp_hist);
}

// The communicator's plane, as cg_scalar_k<MODE, true / false> splits it: the rank's sums into R->v | one all-reduce per
// value, in place | the step on the reduced sums.  TWO: both arrays (the prologue's step and the beta step), else qa alone
template <bool TWO>
__global__ __launch_bounds__(1024) void pcg_local_reduce_k(uint32_t m, const double* __restrict__ qa, const double* __restrict__ qb,
    const PcgScalars* __restrict__ S, PcgRankSums* R)
{
  __shared__ double ldsA[16], ldsB[16];
  const int stopped = S->stop;
  const double ta   = reduce_final_1024(m, qa, ldsA, 1);
  const double tb   = TWO ? reduce_final_1024(m, qb, ldsB, 1) : 0.0;
  if (stopped || threadIdx.x != 0) return;
  R->v[0] = ta;
  if (TWO) R->v[1] = tb;
}
template <int MODE>
__global__ __launch_bounds__(64) void pcg_scalar_reduced_k(PcgScalars* S, const PcgRankSums* __restrict__ R, double* __restrict__ rr_hist,
    double* __restrict__ rz_hist, double* __restrict__ pAp_hist)
{
  const PcgScalars in = pcg_fetch(S);
  const double ta = R->v[0], tb = MODE == 2 ? 0.0 : R->v[1];
  if (in.stop || threadIdx.x != 0) return;
  pcg_apply<MODE>(S, in, ta, tb, rr_hist, rz_hist, pAp_hist);
}

// =============================================================================
// The diagonal, in the device's row order: d_i = the sum, in storage order from +0.0, of row i's stored entries whose column
// is i (both in device numbering; Sell-C-sigma padding is a stored +0.0 and adds +0.0 where its column happens to be the
// row).  One thread per row; correctness kernels, run once per solver handle.  bad[0] counts the rows whose d is not a finite
// positive number, bad[1] holds the first such row (the host presets it to 0xFFFFFFFF).
// =============================================================================
__device__ __forceinline__ void diag_store(uint32_t row, double s, double* __restrict__ d, uint32_t* __restrict__ bad)
{
  d[row] = s;
  if (!(s > 0.0 && s < __builtin_inf())) { // NaN fails both comparisons
    atomicAdd(bad, 1u);
    atomicMin(bad + 1, row);
  }
}
__global__ __launch_bounds__(256) void diag_crs_k(uint32_t nr, const uint32_t* __restrict__ rowPtr, const uint32_t* __restrict__ colInd,
    const double* __restrict__ val, double* __restrict__ d, uint32_t* __restrict__ bad)
{
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= nr) return;
  double s = 0.0;
  for (uint32_t k = rowPtr[row], e = rowPtr[row + 1]; k < e; k++)
    if (colInd[k] == row) s = s + val[k];
  diag_store(row, s, d, bad);
}
__global__ __launch_bounds__(256) void diag_scs_k(uint32_t nr, uint32_t C, const uint32_t* __restrict__ chunkPtr,
    const uint32_t* __restrict__ chunkLens, const uint32_t* __restrict__ colInd, const double* __restrict__ val,
    double* __restrict__ d, uint32_t* __restrict__ bad)
{
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= nr) return;
  const uint32_t chunk = row / C, k = row - chunk * C;
  const uint32_t cp = chunkPtr[chunk], len = chunkLens[chunk];
  double s = 0.0;
  for (uint32_t j = 0; j < len; j++) {
    const size_t idx = (size_t)cp + (size_t)j * C + k;
    if (colInd[idx] == row) s = s + val[idx];
  }
  diag_store(row, s, d, bad);
}
// dinv_i = 1.0 / d_i: one IEEE division (sb_debug_sqrt_div pins the device's division as correctly rounded)
__global__ __launch_bounds__(256) void pcg_reciprocal_k(uint32_t n, const double* __restrict__ d, double* __restrict__ dinv)
{
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dinv[i] = 1.0 / d[i];
}

} // namespace sbk
