// mg.hip.h -- kernels of the multigrid V-cycle preconditioner of PCG beyond its smoother's own (sgs.hip.h): the
// forward sweep that starts from a guess, the residual restricted to the coarse points, the prolongation.  wave64, fp64.
//
// Every operation is rounded on its own (the TU is compiled with -ffp-contract=off): s = s - a * z[col] is one multiply and one
// subtraction, in storage order; z_i = s * dinv_i is one multiply; z_f = z_f + zc_c is one addition.
#pragma once
#include "sgs.hip.h"

namespace sbk {

// The forward sweep of the post-smoother, one colour: chunks [chunk0, chunk0 + nChunks) of the sweep structure, a wave per
// chunk, a lane per row.  z holds a guess:
//   s = r_i - sum lower ;  t_i = s ;  s = s - sum upper ;  z_i = s * dinv_i
// Both halves share slots and rowIdx.  The rows gathered have another colour than the rows written, as in sgs_sweep_k.
__global__ __launch_bounds__(256) void mg_sweep_guess_k(uint32_t chunk0, uint32_t nChunks, const uint32_t* __restrict__ rowIdx,
    SellRows Lo, SellRows Up, const double* __restrict__ r, const double* __restrict__ dinv, double* t, double* z,
    const int* __restrict__ stop)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t ch   = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (*stop) return;
  if (ch >= nChunks) return;
  const uint32_t c   = chunk0 + ch;
  const size_t slot  = (size_t)c * 64u + lane;
  const uint32_t row = rowIdx[slot];
  const bool live    = row != 0xFFFFFFFFu;
  double s           = live ? r[row] : 0.0;
  const double dv    = live ? dinv[row] : 0.0;
  s                  = sell_row<16, false>(Lo, c, lane, Lo.rowLen[slot], z, s);
  if (live) t[row] = s;
  s = sell_row<16, false>(Up, c, lane, Up.rowLen[slot], z, s);
  if (live) z[row] = s * dv;
}

// The restriction structure (built on the host, sbhip_mg.inc.h): Sell-64 over the coarse rows in the coarse level's device
// order.  Per slot the fine device row (0xFFFFFFFF: no row) and the number of its non-zero stored entries, diagonal included;
// col / val of those entries in storage order, column-major per chunk.
struct MgRestrict {
  const unsigned long long* chunkPtr;
  const uint32_t* chunkLen;
  const uint32_t* fineRow;
  const uint32_t* rowLen;
  const uint32_t* col;
  const double* val;
};

// rc_c = r_f - sum over the stored non-zero entries of fine row f = f2c[c] of a * z[col]: the residual at the coarse points
// only.  A wave per chunk, a lane per coarse row; padding is skipped, not multiplied.
__global__ __launch_bounds__(256) void mg_restrict_residual_k(uint32_t nChunks, MgRestrict R, const double* __restrict__ r,
    const double* __restrict__ z, double* __restrict__ rc, const int* __restrict__ stop)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t c    = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (*stop) return;
  if (c >= nChunks) return;
  const size_t slot = (size_t)c * 64u + lane;
  const uint32_t f  = R.fineRow[slot];
  const bool live   = f != 0xFFFFFFFFu;
  const double rf   = live ? r[f] : 0.0;
  const SellRows A  = { R.chunkPtr, R.chunkLen, R.rowLen, R.col, R.val };
  const double s    = sell_row<16, false>(A, c, lane, R.rowLen[slot], z, rf);
  if (live) rc[slot] = s; // (a live slot is a coarse row: slot < the coarse level's rows)
}

// z[f2c[c]] = z[f2c[c]] + zc[c]; the fine rows are distinct, so no two threads touch one element
__global__ __launch_bounds__(256) void mg_prolong_add_k(uint32_t nCoarse, const uint32_t* __restrict__ fineRow,
    const double* __restrict__ zc, double* z, const int* __restrict__ stop)
{
  if (*stop) return;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < nCoarse; c += stride) {
    const uint32_t f = fineRow[c];
    z[f]             = z[f] + zc[c];
  }
}

} // namespace sbk
