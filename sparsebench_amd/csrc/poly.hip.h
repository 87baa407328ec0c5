// poly.hip.h -- kernels of the Chebyshev polynomial preconditioner of PCG: z = q(D^-1 A) D^-1 r, q by the
// Chebyshev recurrence for D^-1 A on [lmin, lmax].  wave64, fp64.
//
// Step 1 is d = z = (r o dinv) * c1; step j >= 2 is w = A z by the matrix's own SpMV, then per row u = r - w, u = u * dinv,
// d = (a_j * d) + (b_j * u), z = z + d.  Every operation is rounded on its own (the TU is compiled with -ffp-contract=off).  The
// coefficients are host doubles passed by value.  The dots r.r and r.z are the canonical dot of kernels.hip.h, their level-1
// values formed from the registers the kernel holds anyway.
// The streaming kernels have the shape of pcg_update_r_k (pcg.hip.h): a wave owns whole aligned 256-row groups (two adjacent
// 128-element spans, lane l holds elements 2l, 2l + 1 of each), the next group's loads go in flight beside the control block,
// the partial last group and an odd n take the guarded loop behind.
#pragma once
#include "kernels.hip.h"
#include "pcg.hip.h"

namespace sbk {

// halves of t0: q0, q1; of t1: q2, q3: the level-1 value of an aligned 256-row group
__device__ __forceinline__ double poly_combine(double t0, double t1)
{
  const double q0 = lane_value<0>(t0), q1 = lane_value<32>(t0), q2 = lane_value<0>(t1), q3 = lane_value<32>(t1);
  return ((q0 + q1) + q2) + q3;
}

// =============================================================================
// The r update with step 1 riding in it, once per body:
//   PRO 0   r = r + (-alpha) Ap ;  d = z = (r o dinv) * c1 ;  level-1 values of r.r        (src = r, coefficient S->neg_alpha)
//   PRO 1   r = b + (-1.0) Ap   ;  the same: the prologue                                   (src = b)
//   LAST 1  steps = 1: z is final, the level-1 values of r.z as well
// A kernel beside pcg_update_r_k and sgs_update_r_k, not a switch inside them.  Seven streams per row (r, Ap, dinv
// in; r, d, z out).
// =============================================================================
template <int PRO, int LAST>
__global__ __launch_bounds__(1024) void poly_update_r_k(uint32_t n, const double* __restrict__ Ap, const double* src, double* r,
    const double* __restrict__ dinv, double* __restrict__ d, double* __restrict__ z, double c1, const PcgScalars* S,
    double* __restrict__ l1rz, double* __restrict__ l1rr)
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
  while (have) {
    const uint32_t e0 = gI * 256u + lane * 2u, e1 = e0 + 128u;
    r0.x = r0.x + c * a0.x, r0.y = r0.y + c * a0.y;
    r1.x = r1.x + c * a1.x, r1.y = r1.y + c * a1.y;
    double2 z0, z1;
    z0.x = pre_first<1>(r0.x, d0.x, c1), z0.y = pre_first<1>(r0.y, d0.y, c1);
    z1.x = pre_first<1>(r1.x, d1.x, c1), z1.y = pre_first<1>(r1.y, d1.y, c1);
    *reinterpret_cast<double2*>(r + e0) = r0;
    *reinterpret_cast<double2*>(r + e1) = r1;
    *reinterpret_cast<double2*>(d + e0) = z0;
    *reinterpret_cast<double2*>(d + e1) = z1;
    *reinterpret_cast<double2*>(z + e0) = z0;
    *reinterpret_cast<double2*>(z + e1) = z1;
    const double vr = poly_combine(butterfly32(r0.x * r0.x + r0.y * r0.y), butterfly32(r1.x * r1.x + r1.y * r1.y));
    if (LAST) {
      const double vz = poly_combine(butterfly32(r0.x * z0.x + r0.y * z0.y), butterfly32(r1.x * z1.x + r1.y * z1.y));
      if (lane == 0) l1rz[gI] = vz;
    }
    if (lane == 0) l1rr[gI] = vr;
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
        zv.x = pre_first<1>(rv.x, dv.x, c1), zv.y = pre_first<1>(rv.y, dv.y, c1);
        *reinterpret_cast<double2*>(r + e) = rv;
        *reinterpret_cast<double2*>(d + e) = zv;
        *reinterpret_cast<double2*>(z + e) = zv;
        sz = rv.x * zv.x + rv.y * zv.y;
        sr = rv.x * rv.x + rv.y * rv.y;
      } else if (e < n) {
        const double rn = src[e] + c * Ap[e];
        const double zn = pre_first<1>(rn, dinv[e], c1);
        r[e] = rn, d[e] = zn, z[e] = zn;
        sz = rn * zn + 0.0;
        sr = rn * rn + 0.0;
      }
      tz[h] = LAST ? butterfly32(sz) : 0.0, tr[h] = butterfly32(sr);
    }
    const double vr = poly_combine(tr[0], tr[1]);
    if (LAST) {
      const double vz = poly_combine(tz[0], tz[1]);
      if (lane == 0) l1rz[gI] = vz;
    }
    if (lane == 0) l1rr[gI] = vr;
  }
}

// =============================================================================
// Step j >= 2 behind w = A z:  u = r - w ;  u = u * dinv ;  d = (a * d) + (b * u) ;  z = z + d.
//   LAST 1  the last step: the level-1 values of r.z from the registers held, so no dot pass follows
// Five streams in (r, w, dinv, d, z), two out (d, z): 56 B per row.  Returns at once when *stop is set.
// =============================================================================
// The kernel's pairs are clang's own two-element vector, not HIP's double2: with ten double2 values carried around the group loop
// this compiler (ROCm's clang for gfx950, -O3) places the first half's new d in the registers that still hold the second half's
// r and w -- wrong results in rows 128 .. 255 of every full group, seen on the device and in the ISA.  With the
// native vector type the allocation is right; the loads and stores are the same global_load / global_store_dwordx4.
typedef double poly_d2 __attribute__((ext_vector_type(2)));
template <int LAST>
__global__ __launch_bounds__(1024) void poly_step_k(uint32_t n, const double* __restrict__ r, const double* __restrict__ w,
    const double* __restrict__ dinv, double* __restrict__ d, double* __restrict__ z, double a, double b,
    double* __restrict__ l1rz, const int* __restrict__ stop)
{
  const uint32_t lane    = threadIdx.x & 63u;
  const uint32_t nGroups = (n + 255u) >> 8;
  const uint32_t nWaves  = gridDim.x * (blockDim.x >> 6);
  uint32_t gI            = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  auto full = [&](uint32_t gg) { return gg < nGroups && gg * 256u + 256u <= n; }; // wave-uniform
  poly_d2 r0, w0, i0, d0, z0, r1, w1, i1, d1, z1; // (set by load before the loop reads them)
  auto load = [&](uint32_t gg) {
    const uint32_t e0 = gg * 256u + lane * 2u, e1 = e0 + 128u;
    r0 = *reinterpret_cast<const poly_d2*>(r + e0), w0 = *reinterpret_cast<const poly_d2*>(w + e0);
    r1 = *reinterpret_cast<const poly_d2*>(r + e1), w1 = *reinterpret_cast<const poly_d2*>(w + e1);
    i0 = *reinterpret_cast<const poly_d2*>(dinv + e0), i1 = *reinterpret_cast<const poly_d2*>(dinv + e1);
    d0 = *reinterpret_cast<const poly_d2*>(d + e0), d1 = *reinterpret_cast<const poly_d2*>(d + e1);
    z0 = *reinterpret_cast<const poly_d2*>(z + e0), z1 = *reinterpret_cast<const poly_d2*>(z + e1);
  };
  auto dir = [&](double rv, double wv, double iv, double dv) { // the new d of one row
    double u = rv - wv;
    u        = u * iv;
    return (a * dv) + (b * u);
  };
  bool have = full(gI);
  if (have) load(gI);
  if (*stop) return;
  while (have) {
    const uint32_t e0 = gI * 256u + lane * 2u, e1 = e0 + 128u;
    poly_d2 nd0, nd1, nz0, nz1;
    nd0.x = dir(r0.x, w0.x, i0.x, d0.x), nd0.y = dir(r0.y, w0.y, i0.y, d0.y);
    nd1.x = dir(r1.x, w1.x, i1.x, d1.x), nd1.y = dir(r1.y, w1.y, i1.y, d1.y);
    nz0.x = z0.x + nd0.x, nz0.y = z0.y + nd0.y;
    nz1.x = z1.x + nd1.x, nz1.y = z1.y + nd1.y;
    *reinterpret_cast<poly_d2*>(d + e0) = nd0;
    *reinterpret_cast<poly_d2*>(d + e1) = nd1;
    *reinterpret_cast<poly_d2*>(z + e0) = nz0;
    *reinterpret_cast<poly_d2*>(z + e1) = nz1;
    if (LAST) {
      const double vz = poly_combine(butterfly32(r0.x * nz0.x + r0.y * nz0.y), butterfly32(r1.x * nz1.x + r1.y * nz1.y));
      if (lane == 0) l1rz[gI] = vz;
    }
    gI += nWaves;
    have = full(gI);
    if (have) load(gI);
  }
  for (; gI < nGroups; gI += nWaves) { // the last, partial group
    double tz[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const uint32_t e = gI * 256u + (uint32_t)h * 128u + lane * 2u;
      double sz        = 0.0;
      if (e + 1 < n) {
        const poly_d2 rv = *reinterpret_cast<const poly_d2*>(r + e);
        const poly_d2 wv = *reinterpret_cast<const poly_d2*>(w + e);
        const poly_d2 iv = *reinterpret_cast<const poly_d2*>(dinv + e);
        const poly_d2 dv = *reinterpret_cast<const poly_d2*>(d + e);
        const poly_d2 zv = *reinterpret_cast<const poly_d2*>(z + e);
        poly_d2 nd, nz;
        nd.x = dir(rv.x, wv.x, iv.x, dv.x), nd.y = dir(rv.y, wv.y, iv.y, dv.y);
        nz.x = zv.x + nd.x, nz.y = zv.y + nd.y;
        *reinterpret_cast<poly_d2*>(d + e) = nd;
        *reinterpret_cast<poly_d2*>(z + e) = nz;
        sz = rv.x * nz.x + rv.y * nz.y;
      } else if (e < n) {
        const double rn = r[e];
        const double dn = dir(rn, w[e], dinv[e], d[e]);
        const double zn = z[e] + dn;
        d[e] = dn, z[e] = zn;
        sz   = rn * zn + 0.0;
      }
      tz[h] = LAST ? butterfly32(sz) : 0.0;
    }
    if (LAST) {
      const double vz = poly_combine(tz[0], tz[1]);
      if (lane == 0) l1rz[gI] = vz;
    }
  }
}

// step 1 outside a solve (sb_pcg_apply_precond, and an apply per multigrid level later): d = z = (r o dinv) * c1; inside a solve
// it rides in poly_update_r_k
__global__ __launch_bounds__(256) void poly_first_k(uint32_t n, const double* __restrict__ r, const double* __restrict__ dinv,
    double* __restrict__ d, double* __restrict__ z, double c1, const int* __restrict__ stop)
{
  if (*stop) return;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double v = pre_first<1>(r[i], dinv[i], c1);
    d[i] = v, z[i] = v;
  }
}

// =============================================================================
// The bound on lmax, in the device's row order: g_i = the sum, in storage order from +0.0 over ALL stored entries e of row i
// (Sell-C-sigma padding is a stored +0.0 and adds +0.0), of (|a_e| * sd_i) * sd[col_e] with sd = sqrt(dinv): an absolute row sum
// of D^-1/2 A D^-1/2.  One thread per row, run once per handle, beside diag_crs_k / diag_scs_k (pcg.hip.h); the host takes the
// maximum.  sqrt is the device's IEEE square root (sb_debug_sqrt_div pins it).
// =============================================================================
__global__ __launch_bounds__(256) void poly_bound_crs_k(uint32_t nr, const uint32_t* __restrict__ rowPtr,
    const uint32_t* __restrict__ colInd, const double* __restrict__ val, const double* __restrict__ dinv, double* __restrict__ gOut)
{
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= nr) return;
  const double sdi = sqrt(dinv[row]);
  double s         = 0.0;
  for (uint32_t k = rowPtr[row], e = rowPtr[row + 1]; k < e; k++) s = s + (fabs(val[k]) * sdi) * sqrt(dinv[colInd[k]]);
  gOut[row] = s;
}
__global__ __launch_bounds__(256) void poly_bound_scs_k(uint32_t nr, uint32_t C, const uint32_t* __restrict__ chunkPtr,
    const uint32_t* __restrict__ chunkLens, const uint32_t* __restrict__ colInd, const double* __restrict__ val,
    const double* __restrict__ dinv, double* __restrict__ gOut)
{
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= nr) return;
  const uint32_t chunk = row / C, k = row - chunk * C;
  const uint32_t cp = chunkPtr[chunk], len = chunkLens[chunk];
  const double sdi = sqrt(dinv[row]);
  double s         = 0.0;
  for (uint32_t j = 0; j < len; j++) {
    const size_t idx = (size_t)cp + (size_t)j * C + k;
    s = s + (fabs(val[idx]) * sdi) * sqrt(dinv[colInd[idx]]);
  }
  gOut[row] = s;
}

} // namespace sbk
