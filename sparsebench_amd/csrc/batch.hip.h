// batch.hip.h -- kernels of batched CG: NV independent CG solves on ONE pass over the matrix.  wave64, fp64.
//
// A block vector is interleaved: element (row, c) sits at X[row * NV + c], rows in the device's row order, NV in {2, 4, 8}
// at compile time.  A lane owns a ROW over all NV columns (one aligned run of 8 NV bytes, read as 16-byte loads; the runs of
// a wave are contiguous), so every dot is formed per column over the same aligned 64-row groups, in the same order, as the
// single-vector kernels form it: level 0 butterfly64 over the group's 64 rows, level 1 ((q0 + q1) + q2) + q3 over the four
// groups of an aligned 256-row block (kernels.hip.h "The canonical dot").  Nothing is added across columns, nothing is
// contracted into an FMA: column c of every kernel here holds the bits the single-vector kernel gives on column c alone.
#pragma once
#include "kernels.hip.h"

namespace sbk {

// the global part of a batched solve's control (the per-column part is CgScalars[NV])
struct CgbControl {
  int stop;     // 1: every column's loop has exited; every kernel returns
  int nStopped; // columns whose loop has exited
};

// one row of a block vector: NV doubles as NV / 2 16-byte accesses
template <int NV> __device__ __forceinline__ void row_load(const double* p, double (&o)[NV])
{
#pragma unroll
  for (int h = 0; h < NV / 2; h++) {
    const double2 t = reinterpret_cast<const double2*>(p)[h];
    o[2 * h] = t.x, o[2 * h + 1] = t.y;
  }
}
template <int NV> __device__ __forceinline__ void row_store(double* p, const double (&v)[NV])
{
#pragma unroll
  for (int h = 0; h < NV / 2; h++) reinterpret_cast<double2*>(p)[h] = double2{ v[2 * h], v[2 * h + 1] };
}

// =============================================================================
// SpMMV, Sell-C-sigma with C = 64, reference layout: the twin of spmv_scs64 (kernels.hip.h) -- same grid, same XCD-aware
// block mapping, same non-temporal matrix loads, one wave per chunk, lane = row.  A val / colInd element is loaded ONCE and
// multiplies the NV values X[col NV .. col NV + NV), gathered as 16-byte loads (neighbouring lanes of a stencil row ask for
// adjacent segments).  scs64_row_sum_block is the twin of scs64_row_sum: per column the products are added left to right in
// the stored order, padding included (0.0 * X[0, c]), exactly as there; it is a twin and not a shared wording because NV
// accumulators per lane change scs64_row_sum's code for the existing kernels.
// =============================================================================
template <int NV, int UNROLL, bool NT>
__device__ __forceinline__ void scs64_row_sum_block(const uint32_t* __restrict__ chunkPtr, const uint32_t* __restrict__ chunkLens,
    const uint32_t* __restrict__ colInd, const double* __restrict__ val, uint32_t chunk, uint32_t lane,
    const double* __restrict__ X, double (&acc)[NV])
{
#pragma unroll
  for (int c = 0; c < NV; c++) acc[c] = 0.0;
  const uint32_t cp  = chunkPtr[chunk];
  const uint32_t len = chunkLens[chunk];
  const double* v    = val + cp + lane;
  const uint32_t* ci = colInd + cp + lane;
  uint32_t j         = 0;
  for (; j + UNROLL <= len; j += UNROLL) {
    double vv[UNROLL];
    uint32_t cc[UNROLL];
    double xx[UNROLL][NV];
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      vv[u] = NT ? stream_load(v + (size_t)(j + u) * 64) : v[(size_t)(j + u) * 64];
      cc[u] = NT ? stream_load(ci + (size_t)(j + u) * 64) : ci[(size_t)(j + u) * 64];
    }
#pragma unroll
    for (int u = 0; u < UNROLL; u++) row_load<NV>(X + (size_t)cc[u] * NV, xx[u]);
#pragma unroll
    for (int u = 0; u < UNROLL; u++)
#pragma unroll
      for (int c = 0; c < NV; c++) acc[c] = acc[c] + vv[u] * xx[u][c];
  }
  for (; j < len; j++) {
    const double vv   = NT ? stream_load(v + (size_t)j * 64) : v[(size_t)j * 64];
    const uint32_t cc = NT ? stream_load(ci + (size_t)j * 64) : ci[(size_t)j * 64];
    double xx[NV];
    row_load<NV>(X + (size_t)cc * NV, xx);
#pragma unroll
    for (int c = 0; c < NV; c++) acc[c] = acc[c] + vv * xx[c];
  }
}

// DOT: column c's level-1 value of X_c . Y_c for the block's four chunks goes to l1[c * nBlocks + lb] -- scs64_block_dot's
// arithmetic per column: the four waves' butterfly64 values meet in LDS, thread c adds ((q0 + q1) + q2) + q3.
template <int NV, int UNROLL, bool DOT, bool NT>
__global__ __launch_bounds__(256) void spmmv_scs64(const uint32_t* __restrict__ chunkPtr,
    const uint32_t* __restrict__ chunkLens, const uint32_t* __restrict__ colInd, const double* __restrict__ val,
    const double* __restrict__ X, double* __restrict__ Y, uint32_t nr, uint32_t nChunks, uint32_t blocksPerXcd,
    double* __restrict__ l1, const int* __restrict__ stop)
{
  const int stopped      = stop ? *stop : 0;
  const uint32_t nBlocks = (nChunks + 3u) >> 2;
  const uint32_t lb      = blocksPerXcd ? xcd_block(blockIdx.x, blocksPerXcd) : blockIdx.x;
  if (lb >= nBlocks || stopped) return; // uniform per workgroup
  const uint32_t chunk = __builtin_amdgcn_readfirstlane(lb * 4u + (threadIdx.x >> 6));
  const uint32_t lane  = threadIdx.x & 63u;
  const bool active    = chunk < nChunks; // wave-uniform; with DOT an idle wave of the last block still joins the combine below
  if (!DOT && !active) return;
  double acc[NV];
#pragma unroll
  for (int c = 0; c < NV; c++) acc[c] = 0.0;
  if (active) scs64_row_sum_block<NV, UNROLL, NT>(chunkPtr, chunkLens, colInd, val, chunk, lane, X, acc);
  const uint32_t row = chunk * 64u + lane;
  const bool mine    = active && row < nr;
  if (mine) row_store<NV>(Y + (size_t)row * NV, acc);
  if (DOT) {
    __shared__ double sq[4][NV];
    double xr[NV];
#pragma unroll
    for (int c = 0; c < NV; c++) xr[c] = 0.0;
    if (mine) row_load<NV>(X + (size_t)row * NV, xr);
#pragma unroll
    for (int c = 0; c < NV; c++) {
      const double t = butterfly64(mine ? xr[c] * acc[c] : 0.0);
      if (lane == 0) sq[threadIdx.x >> 6][c] = t;
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)NV) {
      const uint32_t c                = threadIdx.x;
      l1[(size_t)c * nBlocks + lb] = ((sq[0][c] + sq[1][c]) + sq[2][c]) + sq[3][c];
    }
  }
}

// Every other format (CRS, Sell-C-sigma with C != 64): the correctness kernels, one thread per row, NV accumulators, the
// row's entries in stored order (spmv_crs_* add a row's products left to right from 0.0; spmv_scs_generic walks the padded
// row), no fused dot -- the level-1 values come from block_vec_k<NV, 0> below.  Not tuned.
template <int NV>
__global__ __launch_bounds__(256) void spmmv_crs_rows(const uint32_t* __restrict__ rowPtr, const uint32_t* __restrict__ colInd,
    const double* __restrict__ val, const double* __restrict__ X, double* __restrict__ Y, uint32_t nr,
    const int* __restrict__ stop)
{
  if (stop && *stop) return;
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= nr) return;
  double acc[NV], xx[NV];
#pragma unroll
  for (int c = 0; c < NV; c++) acc[c] = 0.0;
  const uint32_t a = rowPtr[row], b = rowPtr[row + 1];
  for (uint32_t k = a; k < b; k++) {
    const double v = val[k];
    row_load<NV>(X + (size_t)colInd[k] * NV, xx);
#pragma unroll
    for (int c = 0; c < NV; c++) acc[c] = acc[c] + v * xx[c];
  }
  row_store<NV>(Y + (size_t)row * NV, acc);
}
template <int NV>
__global__ __launch_bounds__(256) void spmmv_scs_rows(const uint32_t* __restrict__ chunkPtr,
    const uint32_t* __restrict__ chunkLens, const uint32_t* __restrict__ colInd, const double* __restrict__ val,
    const double* __restrict__ X, double* __restrict__ Y, uint32_t nr, uint32_t nrPadded, uint32_t C,
    const int* __restrict__ stop)
{
  if (stop && *stop) return;
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= nrPadded) return;
  const uint32_t chunk = row / C;
  const uint32_t k     = row - chunk * C;
  const uint32_t cp    = chunkPtr[chunk];
  const uint32_t len   = chunkLens[chunk];
  double acc[NV], xx[NV];
#pragma unroll
  for (int c = 0; c < NV; c++) acc[c] = 0.0;
  for (uint32_t j = 0; j < len; j++) {
    const size_t idx = (size_t)cp + (size_t)j * C + k;
    const double v   = val[idx];
    row_load<NV>(X + (size_t)colInd[idx] * NV, xx);
#pragma unroll
    for (int c = 0; c < NV; c++) acc[c] = acc[c] + v * xx[c];
  }
  if (row < nr) row_store<NV>(Y + (size_t)row * NV, acc);
}

// =============================================================================
// Block vector kernels that produce dots.  A wave owns whole aligned 256-row groups (as dot_l1_k / cg_update_r_k do): four
// steps of 64 rows, lane = row; per column the step's products go through butterfly64 (level 0) and the four values are
// added ((q0 + q1) + q2) + q3 in registers (level 1); lane 0 stores column c's value to l1[c * nGroups + group].  Rows at or
// behind n count as +0.0.
//   OP 0  dot(A_c, B_c)                                   block form of dot_l1_k (the dot pass behind a kernel without one)
//   OP 1  R_c = R_c + (-alpha_c) * A_c ; dot(R_c, R_c)    block form of cg_update_r_k<0> (src/CGSolver.c:128 + :112); A = Ap
//   OP 2  R_c = A_c + (-1.0) * B_c ; dot(R_c, R_c)        block form of dot_spans_k<2> (:97-98); A = b, B = Ap
// OP 1: a column whose loop has exited (S[c].stop) keeps its r, and its level-1 values are not written.
// =============================================================================
template <int NV, int OP>
__global__ __launch_bounds__(256) void block_vec_k(uint32_t n, const double* __restrict__ A, const double* __restrict__ B,
    double* R, const CgScalars* __restrict__ S, double* __restrict__ l1, const int* __restrict__ stop)
{
  const uint32_t lane    = threadIdx.x & 63u;
  const uint32_t nGroups = (n + 255u) >> 8;
  const uint32_t nWaves  = gridDim.x * (blockDim.x >> 6);
  if (stop && *stop) return;
  double nalpha[NV];
  bool live[NV];
#pragma unroll
  for (int c = 0; c < NV; c++) {
    nalpha[c] = OP == 1 ? S[c].neg_alpha : 0.0; // (= -alpha: cg_apply<2> stores both)
    live[c]   = OP == 1 ? S[c].stop == 0 : true;
  }
  for (uint32_t gI = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); gI < nGroups; gI += nWaves) {
    double q[4][NV];
#pragma unroll
    for (int h = 0; h < 4; h++) {
      const uint32_t row = gI * 256u + (uint32_t)h * 64u + lane;
      const bool in      = row < n;
      double a[NV], b[NV], t[NV];
#pragma unroll
      for (int c = 0; c < NV; c++) a[c] = 0.0, b[c] = 0.0;
      if (in) {
        row_load<NV>(A + (size_t)row * NV, a);
        if (OP == 1) row_load<NV>(R + (size_t)row * NV, b);
        else row_load<NV>(B + (size_t)row * NV, b);
      }
      if (OP == 0) {
#pragma unroll
        for (int c = 0; c < NV; c++) t[c] = in ? a[c] * b[c] : 0.0;
      } else {
        double rn[NV];
#pragma unroll
        for (int c = 0; c < NV; c++) {
          if (OP == 1) rn[c] = live[c] ? b[c] + nalpha[c] * a[c] : b[c];
          else rn[c] = a[c] + -1.0 * b[c];
          t[c] = in ? rn[c] * rn[c] : 0.0;
        }
        if (in) row_store<NV>(R + (size_t)row * NV, rn);
      }
#pragma unroll
      for (int c = 0; c < NV; c++) q[h][c] = butterfly64(t[c]);
    }
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < NV; c++)
        if (live[c]) l1[(size_t)c * nGroups + gI] = ((q[0][c] + q[1][c]) + q[2][c]) + q[3][c];
    }
  }
}

// Block form of cg_update_p<0>: P_c = R_c + beta_c * P_c (src/CGSolver.c:114; which != 0: the literal k = 1 form
// P_c = R_c + 0.0 * R_c, :109) and, where column c's previous body left its "x += alpha p" (:127) owing, that update, with
// the old p in registers.  A column whose loop has exited keeps its p and its x (its owed update is cgb_x_finalize's, once).
template <int NV>
__global__ __launch_bounds__(256) void cgb_update_p(uint32_t n, const double* __restrict__ R, double* P, double* X,
    const CgScalars* __restrict__ S, int which, const int* __restrict__ stop)
{
  if (*stop) return;
  double beta[NV], alpha[NV];
  bool live[NV], owed[NV];
  bool anyOwed = false;
#pragma unroll
  for (int c = 0; c < NV; c++) {
    live[c]  = S[c].stop == 0;
    beta[c]  = which == 0 ? S[c].beta : 0.0;
    alpha[c] = S[c].alpha;
    owed[c]  = which == 0 && live[c] && S[c].x_pending != 0;
    anyOwed  = anyOwed || owed[c];
  }
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t row = blockIdx.x * blockDim.x + threadIdx.x; row < n; row += stride) {
    double r[NV], p[NV], x[NV];
    row_load<NV>(R + (size_t)row * NV, r);
    row_load<NV>(P + (size_t)row * NV, p);
    if (anyOwed) {
      row_load<NV>(X + (size_t)row * NV, x);
#pragma unroll
      for (int c = 0; c < NV; c++)
        if (owed[c]) x[c] = x[c] + alpha[c] * p[c];
      row_store<NV>(X + (size_t)row * NV, x);
    }
#pragma unroll
    for (int c = 0; c < NV; c++)
      if (live[c]) p[c] = r[c] + beta[c] * (which == 0 ? p[c] : r[c]);
    row_store<NV>(P + (size_t)row * NV, p);
  }
}

// the owed "x += alpha p" of every column's LAST body (block form of cg_x_finalize): a column's p and alpha have not changed
// since its loop exited
template <int NV>
__global__ __launch_bounds__(256) void cgb_x_finalize(uint32_t n, double* X, const double* __restrict__ P,
    const CgScalars* __restrict__ S)
{
  double alpha[NV];
  bool owed[NV];
  bool any = false;
#pragma unroll
  for (int c = 0; c < NV; c++) alpha[c] = S[c].alpha, owed[c] = S[c].x_pending != 0, any = any || owed[c];
  if (!any) return;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t row = blockIdx.x * blockDim.x + threadIdx.x; row < n; row += stride) {
    double p[NV], x[NV];
    row_load<NV>(P + (size_t)row * NV, p);
    row_load<NV>(X + (size_t)row * NV, x);
#pragma unroll
    for (int c = 0; c < NV; c++)
      if (owed[c]) x[c] = x[c] + alpha[c] * p[c];
    row_store<NV>(X + (size_t)row * NV, x);
  }
}
__global__ void cgb_clear_pending(CgScalars* S, int nv)
{
  if ((int)threadIdx.x < nv) S[threadIdx.x].x_pending = 0;
}

// A scalar step of every column: NV workgroups, workgroup c reduces column c's m level-1 values (reduce_final_1024: level 2
// of the canonical dot) and takes cg_apply<MODE> on column c's control block -- cg_scalar_k<MODE, true> per column.  A column
// whose loop exits counts itself; the last one raises the global stop flag.  Nobody waits for anybody.
template <int MODE>
__global__ __launch_bounds__(1024) void cgb_scalar_k(uint32_t m, const double* __restrict__ l1, CgScalars* S, CgbControl* ctl,
    double* __restrict__ rr_hist, double* __restrict__ pAp_hist, int hist_cap, int defer_x, int nv)
{
  __shared__ double lds16[16];
  const uint32_t c   = blockIdx.x;
  const int allStop  = ctl->stop;
  const CgScalars in = cg_fetch(S + c);
  const double total = reduce_final_1024(m, l1 + (size_t)c * m, lds16, 1);
  if (allStop || in.stop) return;
  if (threadIdx.x == 0) {
    cg_apply<MODE>(S + c, in, total, rr_hist + (size_t)c * hist_cap, pAp_hist + (size_t)c * hist_cap, defer_x);
    const bool exits = MODE == 0 ? !(1 < in.itermax && !!(sqrt(total) > in.eps)) : MODE == 1 ? !(in.iters + 1 < in.itermax && !in.stop_next) : false;
    if (exits && atomicAdd(&ctl->nStopped, 1) == nv - 1) ctl->stop = 1;
  }
}

// =============================================================================
// layout helpers: nrhs plain vectors of n doubles in ORIGINAL row order (vector c at cols + c n) <-> one interleaved block
// vector in the device's row order (perm: newToOld / oldToNew of a permuted Sell-C-sigma matrix, NULL: the same order)
// =============================================================================
__global__ __launch_bounds__(256) void block_interleave_k(uint32_t n, int nv, const uint32_t* __restrict__ newToOld,
    const double* __restrict__ cols, double* __restrict__ X)
{
  const size_t total  = (size_t)n * nv;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const uint32_t row = (uint32_t)(e / nv), c = (uint32_t)(e - (size_t)row * nv);
    X[e] = cols[(size_t)c * n + (newToOld ? newToOld[row] : row)];
  }
}
__global__ __launch_bounds__(256) void block_deinterleave_k(uint32_t n, int nv, const uint32_t* __restrict__ oldToNew,
    const double* __restrict__ X, double* __restrict__ cols)
{
  const size_t total  = (size_t)n * nv;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const uint32_t c = (uint32_t)(e / n), row = (uint32_t)(e - (size_t)c * n);
    cols[e] = X[(size_t)(oldToNew ? oldToNew[row] : row) * nv + c];
  }
}

} // namespace sbk
