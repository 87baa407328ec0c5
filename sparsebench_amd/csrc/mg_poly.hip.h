// mg_poly.hip.h -- kernels of the Chebyshev-smoothed multigrid V-cycle of PCG: the polynomial of poly.hip.h as the
// smoother of every level between mg_fw.hip.h's transfers.  wave64, fp64.
//
// New here are the restriction of the residual that is never written, rc = omega * (P^T (r - w)) with w = A z, and step 1 of the
// post-smoothing from the guess, u = r - w, u = u * dinv, d = u * c1, z = z + d.  Everything else of the cycle is poly.hip.h's
// (poly_update_r_k, poly_first_k, poly_step_k), mg_fw.hip.h's (mg_prolong_p_k) and the matrix's own SpMV.  Every operation is
// rounded on its own (the TU is compiled with -ffp-contract=off).
#pragma once
#include "mg_fw.hip.h"
#include "poly.hip.h"

namespace sbk {

// sell_row<BATCH, true> over the difference of two gathered vectors: s = s + a * (x[col] - y[col]) over a row of `len` entries in
// storage order, the difference formed in registers (one subtraction, one multiply, one addition per entry).  The batching, the
// clamp past the chunk's end and the skip by the lane's own length are sell_row's (sgs.hip.h), which stays as it is: this is a
// loop beside it, not a switch inside it.
template <uint32_t BATCH>
__device__ __forceinline__ double sell_row_diff(uint32_t n, const double* v, const uint32_t* ci, uint32_t len, const double* x,
    const double* y, double s)
{
  for (uint32_t j = 0; j < n; j += BATCH) {
    double a[BATCH], xx[BATCH], yy[BATCH];
    uint32_t cc[BATCH];
#pragma unroll
    for (uint32_t u = 0; u < BATCH; u++) {
      const size_t e = (size_t)min(j + u, n - 1u) * 64u;
      a[u] = stream_load(v + e), cc[u] = stream_load(ci + e);
    }
#pragma unroll
    for (uint32_t u = 0; u < BATCH; u++) xx[u] = x[cc[u]], yy[u] = y[cc[u]];
#pragma unroll
    for (uint32_t u = 0; u < BATCH; u++)
      if (j + u < len) {
        const double t = xx[u] - yy[u];
        s              = s + a[u] * t;
      }
  }
  return s;
}
template <uint32_t BATCH>
__device__ __forceinline__ double sell_row_diff(const SellRows& R, uint32_t c, uint32_t lane, uint32_t len, const double* x,
    const double* y, double s)
{
  return sell_row_diff<BATCH>(R.chunkLen[c], R.val + R.chunkPtr[c] + lane, R.col + R.chunkPtr[c] + lane, len, x, y, s);
}

// rc_c = omega * sum over the kept entries of row c of P^T of w_e * (r[fine row] - w[fine row]), in ascending original fine row
// number (the host's order, mg_fw_sell): mg_restrict_pt_k with the residual formed per entry from its two vectors, so that no
// residual launch runs and no residual vector is written.  A wave per chunk, a lane per coarse row, two batches of 16 for the
// trilinear P's 27 entries.
__global__ __launch_bounds__(256) void mgp_restrict_k(uint32_t nChunks, uint32_t nCoarse, SellRows T, double omega,
    const double* __restrict__ r, const double* __restrict__ w, double* __restrict__ rc, const int* __restrict__ stop)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t c    = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (*stop) return;
  if (c >= nChunks) return;
  const size_t slot = (size_t)c * 64u + lane;
  const double s    = sell_row_diff<16>(T, c, lane, T.rowLen[slot], r, w, 0.0);
  if (slot < nCoarse) rc[slot] = omega * s;
}

// =============================================================================
// Step 1 of the post-smoothing behind w = A z:  u = r - w ;  u = u * dinv ;  d = u * c1 ;  z = z + d.
//   LAST 1  steps = 1 on level 0: z is final, the level-1 values of r.z from the registers held, so no dot pass follows
// poly_step_k's skeleton (a wave owns aligned 256-row groups, 16-byte loads, the guarded tail) and its native vector pairs.  Four
// streams in (r, w, dinv, z), two out (d, z): 48 B per row.  d is only written: a kernel of its own and not poly_step_k with
// a = 0, where 0 * d would be a NaN for a stale inf or NaN in d and +0.0 + -0.0 would lose a sign.  Returns at once when *stop is
// set.
// =============================================================================
template <int LAST>
__global__ __launch_bounds__(1024) void mgp_first_k(uint32_t n, const double* __restrict__ r, const double* __restrict__ w,
    const double* __restrict__ dinv, double* __restrict__ d, double* __restrict__ z, double c1, double* __restrict__ l1rz,
    const int* __restrict__ stop)
{
  const uint32_t lane    = threadIdx.x & 63u;
  const uint32_t nGroups = (n + 255u) >> 8;
  const uint32_t nWaves  = gridDim.x * (blockDim.x >> 6);
  uint32_t gI            = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  auto full = [&](uint32_t gg) { return gg < nGroups && gg * 256u + 256u <= n; }; // wave-uniform
  poly_d2 r0, w0, i0, z0, r1, w1, i1, z1; // (set by load before the loop reads them)
  auto load = [&](uint32_t gg) {
    const uint32_t e0 = gg * 256u + lane * 2u, e1 = e0 + 128u;
    r0 = *reinterpret_cast<const poly_d2*>(r + e0), w0 = *reinterpret_cast<const poly_d2*>(w + e0);
    r1 = *reinterpret_cast<const poly_d2*>(r + e1), w1 = *reinterpret_cast<const poly_d2*>(w + e1);
    i0 = *reinterpret_cast<const poly_d2*>(dinv + e0), i1 = *reinterpret_cast<const poly_d2*>(dinv + e1);
    z0 = *reinterpret_cast<const poly_d2*>(z + e0), z1 = *reinterpret_cast<const poly_d2*>(z + e1);
  };
  auto dir = [&](double rv, double wv, double iv) { // the d of one row
    double u = rv - wv;
    u        = u * iv;
    return u * c1;
  };
  bool have = full(gI);
  if (have) load(gI);
  if (*stop) return;
  while (have) {
    const uint32_t e0 = gI * 256u + lane * 2u, e1 = e0 + 128u;
    poly_d2 nd0, nd1, nz0, nz1;
    nd0.x = dir(r0.x, w0.x, i0.x), nd0.y = dir(r0.y, w0.y, i0.y);
    nd1.x = dir(r1.x, w1.x, i1.x), nd1.y = dir(r1.y, w1.y, i1.y);
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
        const poly_d2 zv = *reinterpret_cast<const poly_d2*>(z + e);
        poly_d2 nd, nz;
        nd.x = dir(rv.x, wv.x, iv.x), nd.y = dir(rv.y, wv.y, iv.y);
        nz.x = zv.x + nd.x, nz.y = zv.y + nd.y;
        *reinterpret_cast<poly_d2*>(d + e) = nd;
        *reinterpret_cast<poly_d2*>(z + e) = nz;
        sz = rv.x * nz.x + rv.y * nz.y;
      } else if (e < n) {
        const double rn = r[e];
        const double dn = dir(rn, w[e], dinv[e]);
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

} // namespace sbk
