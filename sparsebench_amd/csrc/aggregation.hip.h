// aggregation.hip.h -- kernels of the smoothed-aggregation prolongation made from the matrix alone: the strong
// graph of A as a compact neighbour list, the synchronous rounds of a distance-2 maximal independent set on it, the two passes
// that join every other row to a root's aggregate, and the Jacobi smoothing of W = A T into P.  wave64, fp64; a thread per row,
// grids that cover every row (nothing is capped or grid-strided: no launch query).
//
// Nothing here depends on scheduling.  A round reads the keys of its start and writes the next buffer; the only atomic counts
// the rows a round leaves undecided, which steers how many rounds the host enqueues and never a result.  Every floating-point
// operation is rounded on its own (the TU is compiled with -ffp-contract=off).  Vector stores only.
//
// Numbering: the neighbour list, the keys, the aggregates and W are in ORIGINAL numbering; the matrix, its diagonal and dinv are
// in the device's.  A is read in place through galerkin.hip.h's accessors: AggMap::toDev maps an original row to its device row
// and toOrig a device column to its original one (both NULL: the same order).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "galerkin.hip.h"

namespace sbk {

constexpr uint64_t AGG_IN        = 2ull << 62; // the state in bits 62-63 of a key; an out or isolated row's whole key is 0
constexpr uint64_t AGG_UNDECIDED = 1ull << 62;
constexpr uint64_t AGG_STATE     = 3ull << 62;

struct AggMap {
  const uint32_t* toDev;
  const uint32_t* toOrig;
};

// murmur3's 32-bit finaliser
__device__ inline uint32_t agg_fmix32(uint32_t h)
{
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
// the key of row i without its state: 30 hashed bits above the row number, so no two rows share one
__device__ inline uint64_t agg_key(uint32_t i)
{
  const uint32_t h = agg_fmix32((i + 1u) * 0x9E3779B1u);
  return ((uint64_t)(h >> 2) << 32) | (uint64_t)i;
}

// dinv = 1.0 / d in the device's row order; bad = {rows whose d is zero or not finite, the first of them}, preset to
// {0, 0xFFFFFFFF}
__global__ __launch_bounds__(256) void agg_dinv_k(uint32_t n, const double* __restrict__ d, double* __restrict__ dinv,
    uint32_t* __restrict__ bad)
{
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const double v = d[row];
  if (!(v != 0.0 && fabs(v) < INFINITY)) atomicAdd(bad, 1u), atomicMin(bad + 1, row);
  dinv[row] = 1.0 / v;
}

// stored entry e of device row r (original row i) is strong: off the diagonal, not 0.0, a * a > theta^2 * (|d_i| * |d_j|); NaN
// compares false.  Returns the original column, GAL_NONE for an entry that is not strong
template <class X>
__device__ inline uint32_t agg_strong(const X& x, uint32_t r, uint32_t e, uint32_t i, uint32_t n, const uint32_t* toOrig,
    const double* __restrict__ diag, double adi, double theta2)
{
  const size_t k = x.at(r, e);
  const double a = x.val[k];
  const uint32_t c = x.col[k];
  if (c >= n) return GAL_NONE;
  const uint32_t j = toOrig ? toOrig[c] : c;
  if (j == i || !(a != 0.0)) return GAL_NONE;
  return a * a > theta2 * (adi * fabs(diag[c])) ? j : GAL_NONE;
}

// the strong graph, count then fill: FILL = false leaves count[i], FILL = true writes row i's strong columns (original
// numbering, storage order) behind nbrPtr[i].  The rounds gather from this list alone
template <class X, bool FILL>
__global__ __launch_bounds__(256) void agg_graph_k(uint32_t n, X x, AggMap map, const double* __restrict__ diag, double theta2,
    uint32_t* __restrict__ count, const uint32_t* __restrict__ nbrPtr, uint32_t* __restrict__ nbr)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t r   = map.toDev ? map.toDev[i] : i;
  const uint32_t len = x.len(r);
  const double adi   = fabs(diag[r]);
  uint32_t m         = 0;
  const uint32_t o   = FILL ? nbrPtr[i] : 0u;
  const uint32_t cap = FILL ? nbrPtr[i + 1] - o : 0u;
  for (uint32_t e = 0; e < len; e++) {
    const uint32_t j = agg_strong(x, r, e, i, n, map.toOrig, diag, adi, theta2);
    if (j == GAL_NONE) continue;
    if (FILL && m < cap) nbr[o + m] = j;
    m++;
  }
  if (!FILL) count[i] = m;
}

// the keys of the first round's start: undecided, or 0 for an isolated row
__global__ __launch_bounds__(256) void agg_init_k(uint32_t n, const uint32_t* __restrict__ nbrPtr, uint64_t* __restrict__ key)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  key[i] = nbrPtr[i + 1] > nbrPtr[i] ? (agg_key(i) | AGG_UNDECIDED) : 0ull;
}

// out_i = max(in_i, in_j over the strong j of row i)
__device__ inline uint64_t agg_max(uint32_t i, const uint32_t* __restrict__ nbrPtr, const uint32_t* __restrict__ nbr,
    const uint64_t* __restrict__ in)
{
  uint64_t m = in[i];
  for (uint32_t q = nbrPtr[i], e = nbrPtr[i + 1]; q < e; q++) {
    const uint64_t v = in[nbr[q]];
    m                = v > m ? v : m;
  }
  return m;
}

// first half of a round: m1 = the maximum over the row and its strong entries
__global__ __launch_bounds__(256) void agg_propagate_k(uint32_t n, const uint32_t* __restrict__ nbrPtr, const uint32_t* __restrict__ nbr,
    const uint64_t* __restrict__ key, uint64_t* __restrict__ m1)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  m1[i] = agg_max(i, nbrPtr, nbr, key);
}

// second half: m2 over m1, then the decision with the states of the round's start.  An undecided row that holds the largest key
// within two hops becomes in; one that sees an in row there becomes out; the rest stay and are counted in *undecided
__global__ __launch_bounds__(256) void agg_decide_k(uint32_t n, const uint32_t* __restrict__ nbrPtr, const uint32_t* __restrict__ nbr,
    const uint64_t* __restrict__ key, const uint64_t* __restrict__ m1, uint64_t* __restrict__ keyNext, uint32_t* __restrict__ undecided)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = key[i];
  uint64_t out     = k;
  if ((k & AGG_STATE) == AGG_UNDECIDED) {
    const uint64_t m2 = agg_max(i, nbrPtr, nbr, m1);
    if (m2 == k) out = (k & ~AGG_STATE) | AGG_IN;
    else if ((m2 & AGG_STATE) == AGG_IN) out = 0ull;
    else atomicAdd(undecided, 1u);
  }
  keyNext[i] = out;
}

// root[i] = 1 for a row that is in, else 0: what the root numbering is the prefix sum of
__global__ __launch_bounds__(256) void agg_roots_k(uint32_t n, const uint64_t* __restrict__ key, uint32_t* __restrict__ root)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  root[i] = (key[i] & AGG_STATE) == AGG_IN ? 1u : 0u;
}

// pass 1: rootNum[i] is a root's aggregate and -1 for every other row; in1 = rootNum.  A row that is no root takes the largest
// aggregate among its strong entries: pass 1 the root with the largest row (roots are numbered in ascending row), pass 2
// (in1 = pass 1's result) the largest pass-1 aggregate.  A row that has one already keeps it; an isolated row keeps -1
__global__ __launch_bounds__(256) void agg_join_k(uint32_t n, const uint32_t* __restrict__ nbrPtr, const uint32_t* __restrict__ nbr,
    const int32_t* __restrict__ in1, int32_t* __restrict__ out)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int32_t a = in1[i];
  if (a < 0)
    for (uint32_t q = nbrPtr[i], e = nbrPtr[i + 1]; q < e; q++) {
      const int32_t v = in1[nbr[q]];
      a               = v > a ? v : a;
    }
  out[i] = a;
}

// the tentative prolongator's row pointers' increments: 1 for an aggregated row.  left[0] counts the rows that have strong
// entries and still no aggregate (none, by the contract: the host checks)
__global__ __launch_bounds__(256) void agg_check_k(uint32_t n, const uint32_t* __restrict__ nbrPtr, const int32_t* __restrict__ agg,
    uint32_t* __restrict__ left)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (agg[i] < 0 && nbrPtr[i + 1] > nbrPtr[i]) atomicAdd(left, 1u);
}

// P from W = A T in place: P[i, J] = t - (W[i, J] * dinv_i) * s, t = 1.0 where J is row i's aggregate and +0.0 elsewhere.  W in
// original numbering behind 64-bit row pointers, dinv in the device's order
__global__ __launch_bounds__(256) void agg_smooth_k(uint32_t n, const uint64_t* __restrict__ wPtr, const uint32_t* __restrict__ wCol,
    double* __restrict__ wVal, const int32_t* __restrict__ agg, const double* __restrict__ dinv, const uint32_t* __restrict__ toDev,
    double s)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double di  = dinv[toDev ? toDev[i] : i];
  const int32_t ai = agg[i];
  for (uint64_t q = wPtr[i], e = wPtr[i + 1]; q < e; q++) {
    const double t = (ai >= 0 && wCol[q] == (uint32_t)ai) ? 1.0 : 0.0;
    const double u = wVal[q] * di;
    wVal[q]        = t - u * s;
  }
}

} // namespace sbk
