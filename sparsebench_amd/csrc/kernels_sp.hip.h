// kernels_sp.hip.h -- single-precision (CG_FLOAT = float, the reference's FLOAT_TYPE=SP / -DPRECISION=1) kernels of the CG hot
// path for gfx950.  New kernels under new names: the fp64 kernels of kernels.hip.h are untouched.
//
// Every value is a float and every operation a float operation, as the reference's SP build does them (src/util.h:47-51,
// src/matrix-CRS.c:46-60, src/matrix-SCS.c:198-228, src/solver.c:16-62, src/CGSolver.c:63-128): each product is rounded to
// float before its add (-ffp-contract=off: no v_fma_f32), row sums and dot sums accumulate in float.  f32 subnormals are kept
// (hipcc's default kernel mode; never -fgpu-flush-denormals-to-zero or fast-math): the reference's SP histories pass through
// many of them.  Dots use the same fixed tree as fp64 (kernels.hip.h "The canonical dot"), or the reference's sequential sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sbk {

// Control block of the SP CG loop.  rtrans, alpha and normr are float as in src/CGSolver.c:83-84,122; beta is the reference's
// `double beta = rtrans / oldrtrans` (:113): a float division whose float value the double carries into waxpby.
struct CgScalarsF {
  float rr, rr_old, pAp, alpha, neg_alpha, eps;
  double beta;
  int stop, stop_next, iters, n_rr, n_pAp, itermax, hist_cap, x_pending;
  // what the next beta step reads, copied by every alpha step (the beta step at the head of the p update: see CgScalars)
  float snap_rr;
  int snap_iters, snap_stop_next;
};

// ---- fixed-order reductions in float (the fp64 tree, kernels.hip.h) ---------------------------------------------------------
// xor butterfly over the W lanes of an aligned group: every lane ends with the same value
template <int W> __device__ __forceinline__ float xor_sum_f(float v)
{
#pragma unroll
  for (int o = 1; o < W; o <<= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}
// lane l holds elements 4l .. 4l+3 of a 256-group: the butterfly's offsets 1 and 2 are in-lane, 4 .. 32 are lanes xor 1 .. 8;
// lanes 16j .. 16j+15 then hold level-0 partial q_j, and the level-1 value is ((q0 + q1) + q2) + q3
__device__ __forceinline__ float level1_of_lanes_f(float t)
{
  t = xor_sum_f<16>(t);
  const float q0 = __shfl(t, 0, 64), q1 = __shfl(t, 16, 64), q2 = __shfl(t, 32, 64), q3 = __shfl(t, 48, 64);
  return ((q0 + q1) + q2) + q3;
}
__device__ __forceinline__ float in_lane_f(float4 p) { return (p.x + p.y) + (p.z + p.w); }

// levels 1-2 (one workgroup of 1024 threads): thread t adds level-1 values t, t + 1024, ... in order from +0.0, each wave
// butterflies, the 16 wave sums are added in wave order.  q: 4 m level-0 partials, or (l1) the m level-1 values
__device__ __forceinline__ float reduce_final_f32_1024(uint32_t m, const float* __restrict__ q, float* lds16, int l1)
{
  float s = 0.0f;
  for (uint32_t i = threadIdx.x; i < m; i += 1024u)
    s = s + (l1 ? q[i] : ((q[4u * (size_t)i] + q[4u * (size_t)i + 1u]) + q[4u * (size_t)i + 2u]) + q[4u * (size_t)i + 3u]);
  s = xor_sum_f<64>(s);
  if ((threadIdx.x & 63u) == 0) lds16[threadIdx.x >> 6] = s;
  __syncthreads();
  float total = lds16[0];
#pragma unroll
  for (int w = 1; w < 16; w++) total = total + lds16[w];
  return total;
}

// four consecutive elements from e (zeros at and behind n); 16-byte loads where the four lie inside
__device__ __forceinline__ float4 load4_f(const float* p, uint32_t e, uint32_t n)
{
  if (e + 3u < n) return *reinterpret_cast<const float4*>(p + e);
  float4 v = { 0.f, 0.f, 0.f, 0.f };
  if (e < n) v.x = p[e];
  if (e + 1u < n) v.y = p[e + 1u];
  if (e + 2u < n) v.z = p[e + 2u];
  return v;
}
__device__ __forceinline__ void store4_f(float* p, uint32_t e, uint32_t n, float4 v)
{
  if (e + 3u < n) {
    *reinterpret_cast<float4*>(p + e) = v;
    return;
  }
  if (e < n) p[e] = v.x;
  if (e + 1u < n) p[e + 1u] = v.y;
  if (e + 2u < n) p[e + 2u] = v.z;
}
// products a*b of four elements, +0.0 at and behind n
__device__ __forceinline__ float4 prod4_f(float4 a, float4 b, uint32_t e, uint32_t n)
{
  float4 t;
  t.x = e < n ? a.x * b.x : 0.f;
  t.y = e + 1u < n ? a.y * b.y : 0.f;
  t.z = e + 2u < n ? a.z * b.z : 0.f;
  t.w = e + 3u < n ? a.w * b.w : 0.f;
  return t;
}

// ---- SpMV --------------------------------------------------------------------------------------------------------------------
// Sell-C-sigma, C = 64, reference layout (spmv_scs64's counterpart): one wave per chunk, lane = row, non-temporal val / colInd
// streams (256 B of each per wave-instruction), a row summed left to right in float.  DOT: the LEVEL-1 value of x . y for the
// block's four chunks (an aligned 256-group of rows).
template <bool DOT>
__global__ __launch_bounds__(256) void spmv_scs64_f32(const uint32_t* __restrict__ chunkPtr,
    const uint32_t* __restrict__ chunkLens, const uint32_t* __restrict__ colInd, const float* __restrict__ val,
    const float* __restrict__ x, float* __restrict__ y, uint32_t nr, uint32_t nChunks, uint32_t blocksPerXcd,
    float* __restrict__ dotL1, const int* __restrict__ stop)
{
  const int stopped    = stop ? *stop : 0;
  const uint32_t nBlocks = (nChunks + 3u) >> 2;
  const uint32_t lb      = blocksPerXcd ? xcd_block(blockIdx.x, blocksPerXcd) : blockIdx.x;
  if (lb >= nBlocks || stopped) return;
  const uint32_t chunk = __builtin_amdgcn_readfirstlane(lb * 4u + (threadIdx.x >> 6));
  const uint32_t lane  = threadIdx.x & 63u;
  const bool active    = chunk < nChunks;
  if (!DOT && !active) return;
  float acc = 0.0f;
  if (active) acc = scs64_row_sum<4, true>(chunkPtr, chunkLens, colInd, val, chunk, lane, [&](uint32_t col) { return x[col]; });
  const uint32_t row = chunk * 64u + lane;
  if (active && row < nr) y[row] = acc;
  if (DOT) scs64_block_dot((active && row < nr) ? x[row] * acc : 0.0f, lane, dotL1, lb, xor_sum_f<64>);
}

// any C: one thread per padded row
__global__ __launch_bounds__(256) void spmv_scs_generic_f32(const uint32_t* __restrict__ chunkPtr,
    const uint32_t* __restrict__ chunkLens, const uint32_t* __restrict__ colInd, const float* __restrict__ val,
    const float* __restrict__ x, float* __restrict__ y, uint32_t nr, uint32_t nrPadded, uint32_t C, const int* __restrict__ stop)
{
  if (stop && *stop) return;
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= nrPadded) return;
  const uint32_t chunk = row / C, k = row - chunk * C;
  const uint32_t cp = chunkPtr[chunk], len = chunkLens[chunk];
  float acc = 0.0f;
  for (uint32_t j = 0; j < len; j++) {
    const size_t idx = (size_t)cp + (size_t)j * C + k;
    acc              = acc + val[idx] * x[colInd[idx]];
  }
  if (row < nr) y[row] = acc;
}

// CRS, equal nonzero windows (spmv_crs_split's counterpart): tile lb streams [lb T, lb T + 2048), puts the rounded products
// into LDS, and thread r sums row r's products left to right
__global__ __launch_bounds__(CRS_THREADS) void spmv_crs_split_f32(const uint32_t* __restrict__ tileRow,
    const uint32_t* __restrict__ rowPtr, const uint32_t* __restrict__ colInd, const float* __restrict__ val,
    const float* __restrict__ x, float* __restrict__ y, uint32_t nTiles, uint32_t T, uint32_t nnz, uint32_t blocksPerXcd,
    const int* __restrict__ stop)
{
  __shared__ float prod[CRS_TILE];
  const uint32_t lb = xcd_block(blockIdx.x, blocksPerXcd);
  if (lb >= nTiles) return;
  const uint32_t base = lb * T, t = threadIdx.x;
  typedef float flt2 __attribute__((ext_vector_type(2)));
  typedef uint32_t uint2v __attribute__((ext_vector_type(2)));
  constexpr int PAIRS = CRS_BATCH / 2;
  flt2 v[PAIRS], xv[PAIRS];
  uint2v c[PAIRS];
#pragma unroll
  for (int u = 0; u < PAIRS; u++) {
    const uint32_t k = base + 2u * t + (uint32_t)u * 2u * CRS_THREADS;
    v[u] = flt2{ 0.f, 0.f }, c[u] = uint2v{ 0u, 0u };
    if (k < nnz) v[u] = stream_load(reinterpret_cast<const flt2*>(val + k)), c[u] = stream_load(reinterpret_cast<const uint2v*>(colInd + k));
  }
  const int stopped = stop ? *stop : 0;
  const uint32_t r0 = tileRow[lb], r1 = tileRow[lb + 1];
  if (stopped) return;
#pragma unroll
  for (int u = 0; u < PAIRS; u++) xv[u] = flt2{ x[c[u].x], x[c[u].y] };
  uint32_t r = r0 + t, a = 0, b = 0;
  if (r < r1) a = rowPtr[r] - base, b = rowPtr[r + 1] - base;
#pragma unroll
  for (int u = 0; u < PAIRS; u++)
    *reinterpret_cast<flt2*>(&prod[2u * t + (uint32_t)u * 2u * CRS_THREADS]) = flt2{ v[u].x * xv[u].x, v[u].y * xv[u].y };
  __syncthreads();
  while (r < r1) {
    float sum  = 0.0f;
    uint32_t k = a;
    for (; k + 4u <= b; k += 4u) {
      const float d0 = prod[k], d1 = prod[k + 1u], d2 = prod[k + 2u], d3 = prod[k + 3u];
      sum = (((sum + d0) + d1) + d2) + d3;
    }
    for (; k < b; k++) sum = sum + prod[k];
    y[r] = sum;
    r += CRS_THREADS;
    if (r < r1) a = rowPtr[r] - base, b = rowPtr[r + 1] - base;
  }
}

// CRS row blocks (spmv_crs_stream's counterpart): where a row is longer than spmv_crs_split_f32 allows
__global__ __launch_bounds__(CRS_THREADS) void spmv_crs_stream_f32(const uint32_t* __restrict__ rowBlocks,
    const uint32_t* __restrict__ rowPtr, const uint32_t* __restrict__ colInd, const float* __restrict__ val,
    const float* __restrict__ x, float* __restrict__ y, uint32_t nBlocks, uint32_t blocksPerXcd, const int* __restrict__ stop)
{
  __shared__ float prod[CRS_TILE];
  const int stopped = stop ? *stop : 0;
  const uint32_t lb = xcd_block(blockIdx.x, blocksPerXcd);
  if (lb >= nBlocks || stopped) return;
  const uint32_t r0 = rowBlocks[lb], r1 = rowBlocks[lb + 1];
  const uint32_t n0 = rowPtr[r0], n1 = rowPtr[r1];
  const uint32_t t = threadIdx.x;
  auto products = [&](uint32_t lo, uint32_t hi) {
    for (uint32_t k = lo + t; k < hi; k += CRS_THREADS) prod[k - lo] = stream_load(val + k) * x[stream_load(colInd + k)];
  };
  if (n1 - n0 <= (uint32_t)CRS_TILE) {
    products(n0, n1);
    __syncthreads();
    const uint32_t r = r0 + t;
    if (r < r1) {
      float sum = 0.0f;
      for (uint32_t k = rowPtr[r] - n0; k < rowPtr[r + 1] - n0; k++) sum = sum + prod[k];
      y[r] = sum;
    }
  } else { // one row longer than the tile, walked tile by tile in order
    float sum = 0.0f;
    for (uint32_t lo = n0; lo < n1; lo += CRS_TILE) {
      const uint32_t hi = min(lo + (uint32_t)CRS_TILE, n1);
      __syncthreads();
      products(lo, hi);
      __syncthreads();
      if (t == 0)
        for (uint32_t k = 0; k < hi - lo; k++) sum = sum + prod[k];
    }
    if (t == 0) y[r0] = sum;
  }
}

// ---- BLAS-1 --------------------------------------------------------------------------------------------------------------------
// waxpby, src/solver.c:16-39, its three branches as written (w may alias x or y: each element is read before it is written)
__global__ __launch_bounds__(256) void waxpby_f32_k(uint32_t n, float alpha, const float* x, float beta, const float* y, float* w,
    const int* __restrict__ stop)
{
  if (stop && *stop) return;
  const uint32_t stride = gridDim.x * blockDim.x;
  uint32_t i            = blockIdx.x * blockDim.x + threadIdx.x;
  if (alpha == 1.0f)
    for (; i < n; i += stride) w[i] = x[i] + beta * y[i];
  else if (beta == 1.0f)
    for (; i < n; i += stride) w[i] = alpha * x[i] + y[i];
  else
    for (; i < n; i += stride) w[i] = alpha * x[i] + beta * y[i];
}
// w = x + (*a) y with the scalar in HBM (src/CGSolver.c:127-128: waxpby(nrow, 1.0, x, alpha, p, x) takes its first branch)
__global__ __launch_bounds__(256) void axpy_sdev_f32_k(uint32_t n, const float* x, const float* __restrict__ a_dev, const float* y,
    float* w, const int* __restrict__ stop)
{
  if (stop && *stop) return;
  const float a         = *a_dev;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) w[i] = x[i] + a * y[i];
}

// level 0 of the tree dot: one partial per aligned 64 elements (lane = element), 4 ceil(n / 256) of them (tail +0.0)
__global__ __launch_bounds__(256) void dot_l0_f32_k(uint32_t n, const float* __restrict__ a, const float* __restrict__ b,
    float* __restrict__ partials, const int* __restrict__ stop)
{
  if (stop && *stop) return;
  const uint32_t lane = threadIdx.x & 63u, nG = ((n + 255u) >> 8) * 4u, nWaves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t gI = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); gI < nG; gI += nWaves) {
    const uint32_t e = gI * 64u + lane;
    float t          = e < n ? a[e] * b[e] : 0.0f;
    t                = xor_sum_f<64>(t);
    if (lane == 0) partials[gI] = t;
  }
}
// the tree dot as LEVEL-1 values, one per aligned 256 elements (a wave per group; 16-byte aligned operands)
__global__ __launch_bounds__(1024) void dot_l1_f32_k(uint32_t n, const float* __restrict__ a, const float* __restrict__ b,
    float* __restrict__ l1out, const int* __restrict__ stop)
{
  if (stop && *stop) return;
  const uint32_t lane = threadIdx.x & 63u, nG = (n + 255u) >> 8, nWaves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t gI = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); gI < nG; gI += nWaves) {
    const uint32_t e = gI * 256u + lane * 4u;
    const float v    = level1_of_lanes_f(in_lane_f(prod4_f(load4_f(a, e, n), load4_f(b, e, n), e, n)));
    if (lane == 0) l1out[gI] = v;
  }
}
__global__ __launch_bounds__(1024) void reduce_final_f32_k(uint32_t m, const float* __restrict__ q, float* __restrict__ out, int l1)
{
  __shared__ float lds16[16];
  const float total = reduce_final_f32_1024(m, q, lds16, l1);
  if (threadIdx.x == 0) *out = total;
}

// The reference's own order (dot_seq_k's counterpart): `CG_FLOAT sum = 0.0; sum += x[i] * y[i]` over i = 0 .. n-1 (perm: the
// caller's row order over permuted storage), one float chain from +0.0, every product rounded before its add (the products
// cross LDS).  One workgroup: waves 1-15 fill one LDS block while lane 0 of wave 0 adds the other.
constexpr uint32_t DOT_SEQ_F_BLK  = 8192;
constexpr int DOT_SEQ_F_PER       = (DOT_SEQ_F_BLK + DOT_SEQ_PROD - 1) / DOT_SEQ_PROD;
__global__ __launch_bounds__(1024) void dot_seq_f32_k(uint32_t n, const float* __restrict__ a, const float* __restrict__ b,
    const uint32_t* __restrict__ perm, float* __restrict__ out, const int* __restrict__ stop)
{
  __shared__ __attribute__((aligned(16))) float blk[2][DOT_SEQ_F_BLK];
  if (stop && *stop) return;
  const uint32_t nBlk = (uint32_t)(((uint64_t)n + DOT_SEQ_F_BLK - 1) / DOT_SEQ_F_BLK);
  auto count = [&](uint32_t t) { return (uint32_t)min((uint64_t)DOT_SEQ_F_BLK, (uint64_t)n - (uint64_t)t * DOT_SEQ_F_BLK); };
  float sum = 0.0f;
  for (uint32_t t = 0; t <= nBlk; t++) {
    if (threadIdx.x >= 64u) {
      if (t < nBlk) {
        const uint64_t base = (uint64_t)t * DOT_SEQ_F_BLK;
        const uint32_t cnt = count(t), j0 = threadIdx.x - 64u;
        uint32_t k[DOT_SEQ_F_PER];
#pragma unroll
        for (int u = 0; u < DOT_SEQ_F_PER; u++) {
          const uint32_t j = j0 + (uint32_t)u * DOT_SEQ_PROD;
          k[u]             = j < cnt ? (perm ? perm[base + j] : (uint32_t)(base + j)) : 0u;
        }
        float v[DOT_SEQ_F_PER];
#pragma unroll
        for (int u = 0; u < DOT_SEQ_F_PER; u++) v[u] = j0 + (uint32_t)u * DOT_SEQ_PROD < cnt ? a[k[u]] * b[k[u]] : 0.0f;
#pragma unroll
        for (int u = 0; u < DOT_SEQ_F_PER; u++)
          if (j0 + (uint32_t)u * DOT_SEQ_PROD < cnt) blk[t & 1u][j0 + (uint32_t)u * DOT_SEQ_PROD] = v[u];
      }
    } else if (threadIdx.x == 0 && t > 0) {
      const float* src   = blk[(t - 1u) & 1u];
      const uint32_t cnt = count(t - 1u);
      const float4* s4   = reinterpret_cast<const float4*>(src);
      uint32_t j         = 0;
      if (cnt >= 16u) {
        float4 c[4];
#pragma unroll
        for (int u = 0; u < 4; u++) c[u] = s4[u];
        for (j = 16u; j + 16u <= cnt; j += 16u) {
          float4 d[4]; // the next 16 products in flight while the chain adds these
#pragma unroll
          for (int u = 0; u < 4; u++) d[u] = s4[j / 4u + (uint32_t)u];
#pragma unroll
          for (int u = 0; u < 4; u++) sum = (((sum + c[u].x) + c[u].y) + c[u].z) + c[u].w;
#pragma unroll
          for (int u = 0; u < 4; u++) c[u] = d[u];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) sum = (((sum + c[u].x) + c[u].y) + c[u].z) + c[u].w;
      }
      for (; j < cnt; j++) sum = sum + src[j];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = sum;
}

// ---- CG scalar steps with the reference's SP semantics ---------------------------------------------------------------------
// MODE 0: r.r of the prologue and the loop test for k = 1; MODE 1: the loop test for the next k and, if it passes, its r.r and
// beta; MODE 2: p.Ap -> alpha.  normr = sqrt(rtrans) is computed in double and stored to a float (:100,:116); the test is
// `normr > eps` with eps = (CG_FLOAT)param->eps (:64,:107).
__device__ __forceinline__ int sp_normr_fails(float rr, float eps) { return !((float)sqrt((double)rr) > eps); }
template <int MODE>
__device__ __forceinline__ void cg_apply_f32(CgScalarsF* S, const CgScalarsF& in, float total, float* rr_hist, float* pAp_hist,
    int defer_x)
{
  if (MODE == 0) {
    const int sn = sp_normr_fails(total, in.eps);
    S->rr = total, S->stop_next = sn;
    if (in.n_rr < in.hist_cap) rr_hist[in.n_rr] = total;
    S->n_rr = in.n_rr + 1;
    if (1 < in.itermax && !sn) S->iters = 1;
    else S->stop = 1;
  } else if (MODE == 1) {
    if (in.iters + 1 < in.itermax && !in.stop_next) {
      const float old = in.rr;
      S->rr_old = old, S->rr = total;
      S->beta      = (double)(total / old);
      S->stop_next = sp_normr_fails(total, in.eps);
      S->iters     = in.iters + 1;
      if (in.n_rr < in.hist_cap) rr_hist[in.n_rr] = total;
      S->n_rr = in.n_rr + 1;
    } else {
      S->stop = 1;
    }
    if (defer_x) S->x_pending = 1;
  } else {
    S->x_pending = 0;
    S->snap_rr = in.rr, S->snap_iters = in.iters, S->snap_stop_next = in.stop_next;
    S->pAp         = total;
    const float al = in.rr / total;
    S->alpha = al, S->neg_alpha = -al;
    if (in.n_pAp < in.hist_cap) pAp_hist[in.n_pAp] = total;
    S->n_pAp = in.n_pAp + 1;
  }
}

// levels 1-2 of a dot + the scalar step, one workgroup (seq: q[0] is the whole sum, m = 1 and l1 = 1)
template <int MODE>
__global__ __launch_bounds__(1024) void cg_scalar_f32_k(uint32_t m, const float* __restrict__ q, CgScalarsF* S,
    float* __restrict__ rr_hist, float* __restrict__ pAp_hist, int defer_x, int l1)
{
  __shared__ float lds16[16];
  const CgScalarsF in = *S;
  const float total   = reduce_final_f32_1024(m, q, lds16, l1);
  if (in.stop) return;
  if (threadIdx.x == 0) cg_apply_f32<MODE>(S, in, total, rr_hist, pAp_hist, defer_x);
}

// p = r + beta p (src/CGSolver.c:114; which = 1: p = r + 0.0 r, :109) and, x != NULL, the x += alpha p the previous body owes
// (:127).  BETA: the beta step / loop test at the head of the launch, taken by every workgroup from the level-1 values of r.r,
// recorded by workgroup 0 (cg_update_p<1>'s counterpart)
template <int BETA>
__global__ __launch_bounds__(1024) void cg_update_p_f32(uint32_t n, const float* __restrict__ r, float* p, float* x,
    CgScalarsF* S, int which, uint32_t m, const float* __restrict__ rrL1, float* __restrict__ rr_hist)
{
  float beta, alpha;
  bool owed;
  const bool useX = x != nullptr && which == 0;
  if (BETA) {
    __shared__ float lds16[16];
    const bool recorder = blockIdx.x == 0 && threadIdx.x == 0;
    CgScalarsF in;
    if (recorder) in = *S;
    const int stopped = S->stop, iters = S->snap_iters, itermax = S->itermax, stop_next = S->snap_stop_next;
    const float rr    = S->snap_rr;
    alpha             = S->alpha;
    const float total = reduce_final_f32_1024(m, rrL1, lds16, 1);
    if (stopped) return;
    if (recorder && !in.stop) cg_apply_f32<1>(S, in, total, rr_hist, (float*)nullptr, 1);
    if (!(iters + 1 < itermax && !stop_next)) return;
    beta = (float)(double)(total / rr);
    owed = useX;
  } else {
    const int stopped = S->stop;
    beta  = which == 0 ? (float)S->beta : 0.0f;
    owed  = useX && S->x_pending;
    alpha = S->alpha;
    if (stopped) return;
  }
  const uint32_t stride = gridDim.x * blockDim.x * 4u;
  for (uint32_t e = (blockIdx.x * blockDim.x + threadIdx.x) * 4u; e < n; e += stride) {
    const float4 a = load4_f(r, e, n);
    const float4 b = which == 0 ? load4_f(p, e, n) : a;
    if (owed) {
      float4 xv = load4_f(x, e, n);
      xv.x = xv.x + alpha * b.x, xv.y = xv.y + alpha * b.y, xv.z = xv.z + alpha * b.z, xv.w = xv.w + alpha * b.w;
      store4_f(x, e, n, xv);
    }
    float4 o;
    o.x = a.x + beta * b.x, o.y = a.y + beta * b.y, o.z = a.z + beta * b.z, o.w = a.w + beta * b.w;
    store4_f(p, e, n, o);
  }
}

// r = r + (-alpha) Ap (:128) and the level-1 values of the next r.r (a wave per aligned 256 rows).  ALPHA: the alpha step rides
// in this launch -- every workgroup reduces the level-1 values of p.Ap itself, workgroup 0 records (cg_update_r_k<1>'s counterpart)
template <int ALPHA>
__global__ __launch_bounds__(1024) void cg_update_r_f32(uint32_t n, const float* __restrict__ Ap, float* r, CgScalarsF* S,
    float* __restrict__ l1out, const int* stop, uint32_t m, const float* __restrict__ pApL1, float* __restrict__ rr_hist,
    float* __restrict__ pAp_hist)
{
  const uint32_t lane = threadIdx.x & 63u, nG = (n + 255u) >> 8, nWaves = gridDim.x * (blockDim.x >> 6);
  float nalpha;
  if (ALPHA) {
    __shared__ float lds16[16];
    const bool recorder = blockIdx.x == 0 && threadIdx.x == 0;
    CgScalarsF in;
    if (recorder) in = *S;
    const int stopped = S->stop;
    const float rr    = S->rr;
    const float total = reduce_final_f32_1024(m, pApL1, lds16, 1);
    if (stopped) return;
    nalpha = -(rr / total);
    if (recorder) cg_apply_f32<2>(S, in, total, rr_hist, pAp_hist, 0);
  } else {
    if (stop && *stop) return;
    nalpha = S->neg_alpha;
  }
  for (uint32_t gI = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); gI < nG; gI += nWaves) {
    const uint32_t e = gI * 256u + lane * 4u;
    float4 rv        = load4_f(r, e, n);
    const float4 av  = load4_f(Ap, e, n);
    rv.x = rv.x + nalpha * av.x, rv.y = rv.y + nalpha * av.y, rv.z = rv.z + nalpha * av.z, rv.w = rv.w + nalpha * av.w;
    store4_f(r, e, n, rv);
    const float v = level1_of_lanes_f(in_lane_f(prod4_f(rv, rv, e, n)));
    if (lane == 0) l1out[gI] = v;
  }
}

// the x += alpha p the last body that ran still owes
__global__ __launch_bounds__(256) void cg_x_finalize_f32(uint32_t n, float* x, const float* __restrict__ p,
    const CgScalarsF* __restrict__ S)
{
  if (!S->x_pending) return;
  const float alpha     = S->alpha;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] = x[i] + alpha * p[i];
}

__global__ __launch_bounds__(256) void gather_f32_k(uint32_t n, const uint32_t* __restrict__ idx, const float* __restrict__ in,
    float* __restrict__ out)
{
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = in[idx[i]];
}

__global__ __launch_bounds__(256) void max_abs_diff_f32_k(uint32_t n, const float* __restrict__ a, const float* __restrict__ b,
    float* __restrict__ out)
{
  max_abs_diff_block(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, n, a, b, out);
}

} // namespace sbk
