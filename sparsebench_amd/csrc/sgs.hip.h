// sgs.hip.h -- kernels of the symmetric Gauss-Seidel preconditioner of PCG: z = M^-1 r with
// M = (D + L) D^-1 (D + U) in a multicolour order.  wave64, fp64.
//
// Rows of one colour do not couple, so a colour is one launch: forward over the colours 0 .. nC-1 with the entries whose
// column has a smaller colour, backward over nC-2 .. 0 with those of a greater one.  Every operation is rounded on its own
// (the TU is compiled with -ffp-contract=off): s = s - a * z[col] is one multiply and one subtraction, in storage order;
// z_i = s * dinv_i is one multiply.  The forward sums are kept in t, so each sweep reads only its half of the matrix.
//
// The sweep structure (built on the host, sbhip_sgs.inc.h) is Sell-64 per colour: the rows of a colour ascending in chunks of
// 64, val / col column-major per chunk (64 lanes read consecutive addresses), a row index per lane (0xFFFFFFFF: no row) and the
// row's own length, so that padding is skipped, not multiplied: 0.0 * inf would be a NaN the contract does not have.
#pragma once
#include "kernels.hip.h"
#include "pcg.hip.h"

namespace sbk {

// A Sell-64 gather structure: rows in chunks of 64 slots, a wave per chunk, a lane per slot.  The sweeps have two (the lower and
// the upper entries of every row, chunk by chunk), the V-cycle's transfers one each (mg.hip.h, mg_fw.hip.h); the host's one
// packer is sell64_pack (sbhip_sgs.inc.h)
struct SellRows {
  const unsigned long long* chunkPtr; // first element of the chunk in val / col
  const uint32_t* chunkLen;           // longest row of the chunk
  const uint32_t* rowLen;             // per slot: the row's own entries (0 for a slot without a row)
  const uint32_t* col;
  const double* val;
};

// The row loop of every kernel that reads such a structure: s = s - a * z[col] (ADD: s = s + a * z[col]) over a row of `len`
// entries in storage order; v / ci: the lane's first element of val / col, n: the chunk's length (wave-uniform).  BATCH
// elements' loads, then their gathers, in flight before their updates: a stencil's half row (13 entries) is one batch of 16, two
// dependent memory latencies per launch instead of two per entry.  Past the chunk's end the index is clamped to its last element
// (a line already on its way) and the update is skipped by the lane's own length: padding is skipped, not multiplied (0.0 * inf
// would be a NaN the contract does not have).  blockDim / gridDim and the early returns stay in the kernels ("One
// definition per device loop", which also says why sgs_sweep_k below keeps a copy of this loop).
template <uint32_t BATCH, bool ADD>
__device__ __forceinline__ double sell_row(uint32_t n, const double* v, const uint32_t* ci, uint32_t len, const double* z, double s)
{
  for (uint32_t j = 0; j < n; j += BATCH) {
    double a[BATCH], zz[BATCH];
    uint32_t cc[BATCH];
#pragma unroll
    for (uint32_t u = 0; u < BATCH; u++) {
      const size_t e = (size_t)min(j + u, n - 1u) * 64u;
      a[u] = stream_load(v + e), cc[u] = stream_load(ci + e);
    }
#pragma unroll
    for (uint32_t u = 0; u < BATCH; u++) zz[u] = z[cc[u]];
#pragma unroll
    for (uint32_t u = 0; u < BATCH; u++)
      if (j + u < len) s = ADD ? s + a[u] * zz[u] : s - a[u] * zz[u];
  }
  return s;
}
// ... over the row in lane `lane` of chunk c of R
template <uint32_t BATCH, bool ADD>
__device__ __forceinline__ double sell_row(const SellRows& R, uint32_t c, uint32_t lane, uint32_t len, const double* z, double s)
{
  return sell_row<BATCH, ADD>(R.chunkLen[c], R.val + R.chunkPtr[c] + lane, R.col + R.chunkPtr[c] + lane, len, z, s);
}

// One colour: chunks [chunk0, chunk0 + nChunks) of the structure, a wave per chunk, a lane per row.
//   BACKWARD 0   s = r_i - sum lower ;  t_i = s ;  z_i = s * dinv_i
//   BACKWARD 1   s = t_i - sum upper ;             z_i = s * dinv_i
// z is gathered and written in the same launch: the rows gathered have another colour, so no lane reads what another writes
// (a padded element gathers z[0] and drops it).  The matrix stream is read once and does not stay in the caches; t, z, dinv do.
template <int BACKWARD>
__global__ __launch_bounds__(256) void sgs_sweep_k(uint32_t chunk0, uint32_t nChunks, const uint32_t* __restrict__ rowIdx,
    SellRows H, const double* src, const double* __restrict__ dinv, double* t, double* z, const int* __restrict__ stop)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t ch   = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (*stop) return;
  if (ch >= nChunks) return;
  const uint32_t c    = chunk0 + ch;
  const size_t slot   = (size_t)c * 64u + lane;
  const uint32_t row  = rowIdx[slot];
  const uint32_t len  = H.rowLen[slot];
  const uint32_t n    = H.chunkLen[c]; // wave-uniform
  const bool live     = row != 0xFFFFFFFFu;
  const double* v     = H.val + H.chunkPtr[c] + lane;
  const uint32_t* ci  = H.col + H.chunkPtr[c] + lane;
  double s            = live ? src[row] : 0.0;
  const double dv     = live ? dinv[row] : 0.0;
  // sell_row<16, false>(n, v, ci, len, z, s), written out: the twin of that loop, to be changed with it.  Called as a function
  // the loop is compiled ahead of this kernel, its first update stays a branch that the element's loads sink into, and the
  // kernel takes 86 registers for 78
  for (uint32_t j = 0; j < n; j += 16u) {
    double a[16], zz[16];
    uint32_t cc[16];
#pragma unroll
    for (uint32_t u = 0; u < 16u; u++) {
      const size_t e = (size_t)min(j + u, n - 1u) * 64u;
      a[u] = stream_load(v + e), cc[u] = stream_load(ci + e);
    }
#pragma unroll
    for (uint32_t u = 0; u < 16u; u++) zz[u] = z[cc[u]];
#pragma unroll
    for (uint32_t u = 0; u < 16u; u++)
      if (j + u < len) s = s - a[u] * zz[u];
  }
  if (live) {
    if (!BACKWARD) t[row] = s;
    z[row] = s * dv;
  }
}

// z = r o dinv: the diagonal handle's apply outside a solve (sb_pcg_apply_precond); inside one it rides in pcg_update_r_k
__global__ __launch_bounds__(256) void precond_diag_k(uint32_t n, const double* __restrict__ r, const double* __restrict__ dinv,
    double* __restrict__ z)
{
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) z[i] = r[i] * dinv[i];
}

// =============================================================================
// The r update of the SGS path: pcg_update_r_k without z and r.z (z comes from the sweeps, r.z from dot_l1_k behind them).
//   PRO 0   r = r + (-alpha) Ap ;  level-1 values of r.r        (src = r, coefficient S->neg_alpha)
//   PRO 1   r = b + (-1.0) Ap   ;  the same array: the prologue  (src = b)
// A wave owns whole aligned 256-row groups, as there; three streams per row (r, Ap in; r out).
// The twin of pcg_update_r_k (pcg.hip.h), statement for statement less those lines, to be changed with it: as one body with a
// compile-time switch neither kernel keeps its code.
// =============================================================================
template <int PRO>
__global__ __launch_bounds__(1024) void sgs_update_r_k(uint32_t n, const double* __restrict__ Ap, const double* src, double* r,
    const PcgScalars* S, double* __restrict__ l1rr)
{
  const uint32_t lane    = threadIdx.x & 63u;
  const uint32_t nGroups = (n + 255u) >> 8;
  const uint32_t nWaves  = gridDim.x * (blockDim.x >> 6);
  uint32_t gI            = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  auto full = [&](uint32_t gg) { return gg < nGroups && gg * 256u + 256u <= n; }; // wave-uniform
  double2 r0 = { 0.0, 0.0 }, a0 = r0, r1 = r0, a1 = r0;
  auto load = [&](uint32_t gg) {
    const uint32_t e0 = gg * 256u + lane * 2u, e1 = e0 + 128u;
    r0 = *reinterpret_cast<const double2*>(src + e0), a0 = *reinterpret_cast<const double2*>(Ap + e0);
    r1 = *reinterpret_cast<const double2*>(src + e1), a1 = *reinterpret_cast<const double2*>(Ap + e1);
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
    *reinterpret_cast<double2*>(r + e0) = r0;
    *reinterpret_cast<double2*>(r + e1) = r1;
    const double vr = combine(butterfly32(r0.x * r0.x + r0.y * r0.y), butterfly32(r1.x * r1.x + r1.y * r1.y));
    if (lane == 0) l1rr[gI] = vr;
    gI += nWaves;
    have = full(gI);
    if (have) load(gI);
  }
  for (; gI < nGroups; gI += nWaves) { // the last, partial group
    double tr[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const uint32_t e = gI * 256u + (uint32_t)h * 128u + lane * 2u;
      double sr        = 0.0;
      if (e + 1 < n) {
        double2 rv       = *reinterpret_cast<const double2*>(src + e);
        const double2 av = *reinterpret_cast<const double2*>(Ap + e);
        rv.x = rv.x + c * av.x;
        rv.y = rv.y + c * av.y;
        *reinterpret_cast<double2*>(r + e) = rv;
        sr = rv.x * rv.x + rv.y * rv.y;
      } else if (e < n) {
        const double rn = src[e] + c * Ap[e];
        r[e]            = rn;
        sr              = rn * rn + 0.0;
      }
      tr[h] = butterfly32(sr);
    }
    const double vr = combine(tr[0], tr[1]);
    if (lane == 0) l1rr[gI] = vr;
  }
}

} // namespace sbk
