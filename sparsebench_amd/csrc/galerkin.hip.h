// galerkin.hip.h -- kernels of the sparse triple product A_c = P^T A P: both stages are one row-wise product
// C = X Y in which every output entry is a SEQUENTIAL sum over the terms of its row, in X's row order and, inside one entry of
// X, in the storage order of Y's row.  wave64, fp64, a wave (one 64-thread workgroup) per output row.
//
// Every operation is rounded on its own (the TU is compiled with -ffp-contract=off): t = x * y is one multiply, s = s + t one
// addition, s starts from +0.0.  The parallelism never changes the order of the additions of one entry: the lanes form the
// products of 64 terms at once and park them in LDS in TERM ORDER, then the lane that owns an output column walks the parked
// terms front to back and adds those of its column.  No atomics on values, vector stores only.
//
// Two launches per stage: gal_count_k finds how many distinct columns each output row has (the host turns the counts into the
// 64-bit row pointers), gal_fill_k finds them again, sorts them and writes columns and sums.  The set of a row's columns is a
// dense list in LDS filled in arrival order (a new column is one that is neither in the list nor held by a lower lane of the
// same 64 terms); at most GAL_CAP of them, a row with more is reported, never truncated.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sbk {

constexpr uint32_t GAL_CAP  = 1024u;       // distinct columns of one output row
constexpr uint32_t GAL_NONE = 0xFFFFFFFFu; // a term that does not count (a stored 0.0 weight, a lane past the last term)

// X: entry e of row d.  The device matrix in place in the reference's layout (CRS, Sell-C-sigma), or P^T as 64-bit CSR
struct GalCrs {
  const uint32_t* rowPtr;
  const uint32_t* col;
  const double* val;
  __device__ uint32_t len(uint32_t d) const { return rowPtr[d + 1] - rowPtr[d]; }
  __device__ size_t at(uint32_t d, uint32_t e) const { return (size_t)rowPtr[d] + e; }
};
struct GalSell {
  const uint32_t* chunkPtr;
  const uint32_t* chunkLens;
  uint32_t C;
  const uint32_t* col;
  const double* val;
  __device__ uint32_t len(uint32_t d) const { return chunkLens[d / C]; }
  __device__ size_t at(uint32_t d, uint32_t e) const { return (size_t)chunkPtr[d / C] + (size_t)e * C + d % C; }
};
struct GalCsr64 {
  const uint64_t* ptr;
  const uint32_t* col;
  const double* val;
  __device__ uint32_t len(uint32_t d) const { return (uint32_t)(ptr[d + 1] - ptr[d]); }
  __device__ size_t at(uint32_t d, uint32_t e) const { return (size_t)ptr[d] + e; }
};
// Y: 64-bit CSR, nY rows
struct GalY {
  const uint64_t* ptr;
  const uint32_t* col;
  const double* val;
  uint32_t nY;
};
// which rows: output row i is X's row rowOf[i], X's column c is Y's row colMap[c] (NULL: the identity) -- a permuted
// Sell-C-sigma matrix is read in its device numbering and written in the original one
struct GalMap {
  const uint32_t* rowOf;
  const uint32_t* colMap;
};

struct GalLds {
  uint32_t list[GAL_CAP];   // the row's distinct columns in arrival order
  uint32_t sorted[GAL_CAP]; // ... ascending
  uint64_t xbase[64];       // per entry of the X tile: its Y row's first entry,
  double xa[64];            // its value,
  uint32_t xoff[65];        // and the number of its first term among the tile's (exclusive prefix; [64] the total)
  uint32_t tcol[64];        // 64 terms in term order: column (GAL_NONE: none) and product
  double tval[64];
};

// the X tile of entries e0 .. e0 + 63 of row d into LDS; returns the tile's terms.  An entry whose stored value compares equal
// to 0.0 has no terms (Sell padding and explicit zeros alike).  A column outside Y's rows sets *bad and has no terms.
template <class X>
__device__ uint32_t gal_xtile(const X& x, uint32_t d, uint32_t e0, uint32_t len, const GalMap& map, const GalY& y, GalLds& L,
    uint32_t lane, unsigned int* bad)
{
  const uint32_t e = e0 + lane;
  uint32_t ylen    = 0;
  uint64_t yb      = 0;
  double a         = 0.0;
  if (e < len) {
    const size_t k = x.at(d, e);
    a              = x.val[k];
    if (a != 0.0) {
      uint32_t c = x.col[k];
      if (c < y.nY) {
        if (map.colMap) c = map.colMap[c];
        yb   = y.ptr[c];
        ylen = (uint32_t)(y.ptr[c + 1] - yb);
      } else {
        atomicOr(bad, 1u);
      }
    }
  }
  uint32_t inc = ylen;
  for (uint32_t o = 1; o < 64u; o <<= 1) {
    const uint32_t v = __shfl_up(inc, o);
    if (lane >= o) inc += v;
  }
  __syncthreads(); // the tile before this one has been read
  L.xoff[lane] = inc - ylen, L.xbase[lane] = yb, L.xa[lane] = a;
  if (lane == 63u) L.xoff[64] = inc;
  __syncthreads();
  return L.xoff[64];
}

// term t of the tile (t < its total): the entry of X it belongs to is the last whose first term is not behind t
template <bool SKIPY> __device__ void gal_term(const GalLds& L, const GalY& y, uint32_t t, uint32_t& col, double& prod)
{
  uint32_t j = 0;
  for (uint32_t s = 32; s; s >>= 1)
    if (L.xoff[j + s] <= t) j += s;
  const size_t q = (size_t)L.xbase[j] + (t - L.xoff[j]);
  const double w = y.val[q];
  col            = (SKIPY && w == 0.0) ? GAL_NONE : y.col[q];
  prod           = L.xa[j] * w;
}

// the distinct columns of output row `row` into L.list (arrival order); returns their count, which is above GAL_CAP exactly
// when the row does not fit (the list then holds the first GAL_CAP)
template <class X, bool SKIPY>
__device__ uint32_t gal_columns(const X& x, uint32_t d, uint32_t len, const GalMap& map, const GalY& y, GalLds& L, uint32_t lane,
    unsigned int* bad)
{
  uint32_t n = 0;
  for (uint32_t e0 = 0; e0 < len; e0 += 64u) {
    const uint32_t total = gal_xtile(x, d, e0, len, map, y, L, lane, bad);
    for (uint32_t t0 = 0; t0 < total; t0 += 64u) {
      uint32_t col = GAL_NONE;
      double prod;
      if (t0 + lane < total) gal_term<SKIPY>(L, y, t0 + lane, col, prod);
      __syncthreads();
      L.tcol[lane] = col;
      __syncthreads();
      bool fresh = col != GAL_NONE;
      for (uint32_t k = 0; k < n; k++)
        if (L.list[k] == col) fresh = false;
      for (uint32_t k = 0; k < 64u; k++)
        if (k < lane && L.tcol[k] == col) fresh = false;
      const unsigned long long m = __ballot(fresh);
      const uint32_t pos         = n + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      if (fresh && pos < GAL_CAP) L.list[pos] = col;
      __syncthreads();
      n += (uint32_t)__popcll(m);
      if (n > GAL_CAP) return n;
    }
  }
  return n;
}

// count[i] = distinct columns of output row i; a row above GAL_CAP leaves (row << 32 | count reached) in *over (the smallest
// such row wins: atomicMin) and a count of 0
template <class X, bool SKIPY>
__global__ __launch_bounds__(64) void gal_count_k(uint32_t nRows, X x, GalMap map, GalY y, uint32_t* __restrict__ count,
    unsigned long long* __restrict__ over, unsigned int* __restrict__ bad)
{
  __shared__ GalLds L;
  const uint32_t lane = threadIdx.x, row = blockIdx.x;
  if (row >= nRows) return;
  const uint32_t d   = map.rowOf ? map.rowOf[row] : row;
  const uint32_t len = x.len(d);
  uint32_t n         = gal_columns<X, SKIPY>(x, d, len, map, y, L, lane, bad);
  if (n > GAL_CAP) {
    if (lane == 0) atomicMin(over, ((unsigned long long)row << 32) | n);
    n = 0;
  }
  if (lane == 0) count[row] = n;
}

// columns (ascending) and sums of output row i behind outPtr[i]; outPtr[i + 1] - outPtr[i] is gal_count_k's count
template <class X, bool SKIPY>
__global__ __launch_bounds__(64) void gal_fill_k(uint32_t nRows, X x, GalMap map, GalY y, const uint64_t* __restrict__ outPtr,
    uint32_t* __restrict__ outCol, double* __restrict__ outVal, unsigned int* __restrict__ bad)
{
  __shared__ GalLds L;
  const uint32_t lane = threadIdx.x, row = blockIdx.x;
  if (row >= nRows) return;
  const uint32_t d   = map.rowOf ? map.rowOf[row] : row;
  const uint32_t len = x.len(d);
  const uint64_t o   = outPtr[row];
  const uint32_t n   = gal_columns<X, SKIPY>(x, d, len, map, y, L, lane, bad);
  if (n > GAL_CAP || (uint64_t)n != outPtr[row + 1] - o) { // (cannot happen behind gal_count_k: nothing is written then)
    atomicOr(bad, 2u);
    return;
  }
  // ascending: every column's rank is the number of smaller ones (they are distinct)
  for (uint32_t k = lane; k < n; k += 64u) {
    const uint32_t key = L.list[k];
    uint32_t r         = 0;
    for (uint32_t j = 0; j < n; j++) r += L.list[j] < key ? 1u : 0u;
    L.sorted[r] = key;
  }
  __syncthreads();
  // lane c owns output column c, in rounds of 64; the terms are walked again per round
  for (uint32_t c0 = 0; c0 < n; c0 += 64u) {
    const bool own     = c0 + lane < n;
    const uint32_t key = own ? L.sorted[c0 + lane] : GAL_NONE;
    double s           = 0.0;
    for (uint32_t e0 = 0; e0 < len; e0 += 64u) {
      const uint32_t total = gal_xtile(x, d, e0, len, map, y, L, lane, bad);
      for (uint32_t t0 = 0; t0 < total; t0 += 64u) {
        uint32_t col = GAL_NONE;
        double prod  = 0.0;
        if (t0 + lane < total) gal_term<SKIPY>(L, y, t0 + lane, col, prod);
        __syncthreads();
        L.tcol[lane] = col, L.tval[lane] = prod;
        __syncthreads();
        const uint32_t cnt = total - t0 < 64u ? total - t0 : 64u;
        for (uint32_t k = 0; k < cnt; k++)
          if (own && L.tcol[k] == key) s = s + L.tval[k];
      }
    }
    if (own) outCol[o + c0 + lane] = key, outVal[o + c0 + lane] = s;
  }
}

} // namespace sbk
