// mg_fw.hip.h -- kernels of the full-weighting transfers of the multigrid V-cycle beside mg.hip.h's injection: the
// full residual d = r - A z in one launch, the restriction rc = omega * (P^T d), the prolongation z = z + P zc.  wave64, fp64.
//
// Every operation is rounded on its own (the TU is compiled with -ffp-contract=off): s = s - a * z[col] and s = s + w * d[col]
// are one multiply and one subtraction or addition, in the structure's storage order; rc_c = omega * s is one multiply;
// z_i = z_i + s is one addition.
#pragma once
#include "mg.hip.h"

namespace sbk {

// d_i = r_i - sum lower - sum upper - diag_i * z_i over every row of the level: all chunks of all colours of the sweep structure
// in ONE launch (a residual has no colour dependence), a wave per chunk, a lane per row.  Both halves are read with sell_row's
// batching and skip-by-own-length rule.  z is only read here, d only written: no lane reads what another writes.
__global__ __launch_bounds__(256) void mg_residual_k(uint32_t nChunks, const uint32_t* __restrict__ rowIdx, SellRows Lo, SellRows Up,
    const double* __restrict__ r, const double* __restrict__ z, const double* __restrict__ diag, double* __restrict__ d,
    const int* __restrict__ stop)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t c    = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (*stop) return;
  if (c >= nChunks) return;
  const size_t slot  = (size_t)c * 64u + lane;
  const uint32_t row = rowIdx[slot];
  const bool live    = row != 0xFFFFFFFFu;
  double s           = live ? r[row] : 0.0;
  const double dg    = live ? diag[row] : 0.0;
  const double zi    = live ? z[row] : 0.0;
  s                  = sell_row<16, false>(Lo, c, lane, Lo.rowLen[slot], z, s);
  s                  = sell_row<16, false>(Up, c, lane, Up.rowLen[slot], z, s);
  if (live) d[row] = s - dg * zi;
}

// A transfer operator (built on the host, sbhip_mg_fw.inc.h) is a SellRows over the rows written, in their level's device order
// (slot == device row), the columns the device rows of the level gathered from; rowLen per slot is the row's kept (non-zero)
// entries, 0 for a row without any and for a slot past the last row.  Its sums start from +0.0 and add: sell_row<BATCH, true>

// rc_c = omega * sum over the kept entries of row c of P^T of w * d[fine row], in ascending original fine row number (the
// host's order): a wave per chunk, a lane per coarse row.  The trilinear P has up to 27 entries per row: two batches of 16.
__global__ __launch_bounds__(256) void mg_restrict_pt_k(uint32_t nChunks, uint32_t nCoarse, SellRows T, double omega,
    const double* __restrict__ d, double* __restrict__ rc, const int* __restrict__ stop)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t c    = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (*stop) return;
  if (c >= nChunks) return;
  const size_t slot = (size_t)c * 64u + lane;
  const double s    = sell_row<16, true>(T, c, lane, T.rowLen[slot], d, 0.0);
  if (slot < nCoarse) rc[slot] = omega * s;
}

// z_i = z_i + sum over the kept entries of row i of P of w * zc[coarse row], in the caller's storage order; a row without a kept
// entry writes nothing.  A wave per chunk, a lane per fine row; up to 8 entries per row for the trilinear P: one batch.
__global__ __launch_bounds__(256) void mg_prolong_p_k(uint32_t nChunks, SellRows T, const double* __restrict__ zc, double* z,
    const int* __restrict__ stop)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t c    = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (*stop) return;
  if (c >= nChunks) return;
  const size_t slot  = (size_t)c * 64u + lane;
  const uint32_t len = T.rowLen[slot];
  const double s     = sell_row<8, true>(T, c, lane, len, zc, 0.0);
  if (len) z[slot] = z[slot] + s; // (len > 0 only for slot < the level's rows)
}

} // namespace sbk
