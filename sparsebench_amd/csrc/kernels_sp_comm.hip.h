// kernels_sp_comm.hip.h -- single precision on several ranks: the in-kernel float all-reduce, the f32 halo push / pull over
// peer-mapped memory, and the pieces of the communicator's plane (local reduce | all-reduce | apply; halo pack / unpack).
// The fp64 protocol of kernels.hip.h (P2PSlot / P2PView slots, sequence numbers, parities, bounded waits, P2P_POISON, the
// last-workgroup flag release) with float payloads.  New kernels under new names: the fp64 kernels and the one-rank fp32
// kernels of kernels_sp.hip.h are untouched (CgScalarsF keeps its layout; the multi-rank state lives in CgCommF).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sbk {

// what the SP loop needs on several ranks next to its control block (CgScalars::local / p2p_error of the fp64 loop)
struct CgCommF {
  float local;   // rank-local sum handed to / returned by the communicator's all-reduce
  int p2p_error; // 1: a peer's contribution to an in-kernel all-reduce did not arrive in time, 2: a peer reported a failure
};

// The rank sum of the reference's MPI_Allreduce(MPI_FLOAT, SUM) as MPICH adds it: pairwise in rank order,
// ((v0 + v1) + (v2 + v3)) + ..., an odd tail moving up unchanged; every add a float add (no FMA, f32 subnormals kept).
// op 0: MAX, in rank order.  In place over v[0 .. P); returns the result.  Host (transport) and device (both planes) alike.
__host__ __device__ inline float rank_reduce_f32(float* v, int P, int op)
{
  if (op == 0) {
    float m = v[0];
    for (int i = 1; i < P; i++)
      if (v[i] > m) m = v[i];
    return m;
  }
  int n = P;
  while (n > 1) {
    const int h = n >> 1;
    for (int i = 0; i < h; i++) v[i] = v[2 * i] + v[2 * i + 1];
    if (n & 1) v[h] = v[n - 1];
    n = h + (n & 1);
  }
  return v[0];
}

// p2p_allreduce_sum with a float payload: the float's bits in the low half of P2PSlot::bits.  Every thread of the workgroup
// calls it with the same `mine`; returns the same sum in every thread.  sh: >= P2P_MAX floats of LDS.
__device__ __forceinline__ float p2p_allreduce_sum_f32(const P2PView* pv, float mine, unsigned long long seq, float* sh, int* err)
{
  const int t = (int)threadIdx.x, P = pv->size;
  p2p_exchange(pv, mine, seq, sh, err);
  if (t == 0) sh[0] = rank_reduce_f32(sh, P, 1);
  __syncthreads();
  const float r = sh[0];
  __syncthreads();
  return r;
}

// cg_scalar_p2p_k in float: local levels 1-2 (seq: q[0], m = 1), the exchange, the SP step (cg_apply_f32) -- one launch
template <int MODE>
__global__ __launch_bounds__(1024) void cg_scalar_p2p_f32_k(uint32_t m, const float* __restrict__ q, CgScalarsF* S, CgCommF* X,
    float* __restrict__ rr_hist, float* __restrict__ pAp_hist, int defer_x, const P2PView* __restrict__ pv, unsigned long long seq,
    int l1, const int* __restrict__ haloErr)
{
  __shared__ float lds16[P2P_MAX];
  const CgScalarsF in = *S;
  const int stopped   = in.stop; // identical on every rank -- unless one has failed
  float total         = reduce_final_f32_1024(m, q, lds16, l1);
  if (stopped) {
    if (X->p2p_error || (haloErr && *haloErr)) p2p_poison_allreduce(pv); // this rank has failed: nobody waits for it
    return;
  }
  __syncthreads(); // lds16 is reused
  total = p2p_allreduce_sum_f32(pv, total, seq, lds16, &X->p2p_error);
  if (__hip_atomic_load(&X->p2p_error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { // uniform: raised before the barriers
    if (threadIdx.x == 0) S->stop = 1;
    p2p_poison_allreduce(pv);
    return;
  }
  if (threadIdx.x == 0) cg_apply_f32<MODE>(S, in, total, rr_hist, pAp_hist, defer_x);
}

// the communicator's plane, split (cg_scalar_k<MODE, true / false> of fp64): levels 1-2 of the rank's dot into X->local ...
__global__ __launch_bounds__(1024) void cg_local_f32_k(uint32_t m, const float* __restrict__ q, const CgScalarsF* __restrict__ S,
    CgCommF* X, int l1)
{
  __shared__ float lds16[16];
  const int stopped = S->stop;
  const float total = reduce_final_f32_1024(m, q, lds16, l1);
  if (stopped) return;
  if (threadIdx.x == 0) X->local = total;
}
// ... and, behind the all-reduce of X->local, the SP step on the all-reduced value
template <int MODE>
__global__ __launch_bounds__(64) void cg_apply_local_f32_k(CgScalarsF* S, const CgCommF* __restrict__ X, float* __restrict__ rr_hist,
    float* __restrict__ pAp_hist, int defer_x)
{
  if (threadIdx.x != 0) return;
  const CgScalarsF in = *S;
  if (in.stop) return;
  cg_apply_f32<MODE>(S, in, X->local, rr_hist, pAp_hist, defer_x);
}

// RCCL's all-gather of the P rank values, then the rank tree (one thread: P adds)
__global__ __launch_bounds__(64) void rank_reduce_f32_k(float* all, int P, int op, float* out)
{
  if (threadIdx.x == 0) *out = rank_reduce_f32(all, P, op);
}

// halo_push_k with float values: x[packIdx[i]] in the vector's device order; each float's bits go into the low half of the
// receiver's 64-bit staging slot (the same [2][externalCount] x 8 B area and slot numbers as fp64).  The last workgroup raises
// the flags (system-scope release); a stopped rank that has failed poisons them instead.
__global__ __launch_bounds__(256) void halo_push_f32_k(HaloPush hp, const float* __restrict__ x, unsigned long long seq,
    const int* __restrict__ stop)
{
  if (stop && *stop) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && halo_rank_failed(hp)) halo_poison_flags(hp);
    return;
  }
  halo_push_block(hp, x, seq, blockIdx.x, gridDim.x);
}

// halo_pull_k into the float tail of p: one workgroup per source, bounded wait on its flag, then the block
__global__ __launch_bounds__(256) void halo_pull_f32_k(const int* __restrict__ srcRank, const int* __restrict__ rdispl,
    const int* __restrict__ rcount, const unsigned long long* stage, const unsigned long long* flags, uint32_t ext,
    float* __restrict__ xTail, unsigned long long seq, int* err, int* stop, long long timeoutTicks)
{
  if (stop && *stop) return;
  halo_pull_block(srcRank, rdispl, rcount, stage, flags, ext, xTail, seq, err, stop, timeoutTicks);
}

// ---- the halo exchange folded into the loop's own kernels (sb_comm_halo_fold; kernels.hip.h: cg_update_p_push,
// spmv_scs64_halo) in float.  One halo plan and one HaloFold / ScsHalo plan serve both precisions: they hold indices only,
// and a float travels in the low half of its 64-bit staging slot, as halo_push_f32_k sends it.
// cg_update_p_f32<0> + the push of the rows each workgroup has written (the plan's owner map follows THIS kernel's
// four-elements-per-thread grid)
__global__ __launch_bounds__(1024) void cg_update_p_push_f32(HaloPush hp, HaloFold hf, unsigned long long seq, uint32_t n,
    const float* __restrict__ r, float* p, float* x, CgScalarsF* S, int which)
{
  const bool useX   = x != nullptr && which == 0;
  const int stopped = S->stop;
  const float beta  = which == 0 ? (float)S->beta : 0.0f;
  const bool owed   = useX && S->x_pending;
  const float alpha = S->alpha;
  if (stopped) { // the same decision on every rank -- unless this rank has failed
    if (blockIdx.x == 0 && threadIdx.x == 0 && halo_rank_failed(hp)) halo_poison_flags(hp);
    return;
  }
  // A copy of cg_update_p_f32's sweep, which it must agree with (as one shared function it changes this kernel's code:
  // DESIGN 4.6).
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
  const uint32_t e0 = hf.wgStart[blockIdx.x], e1 = hf.wgStart[blockIdx.x + 1u];
  if (e0 == e1) return; // (uniform per workgroup)
  halo_fold_push(hp, hf, seq, p, e0, e1, blockDim.x);
}

// spmv_scs64_f32<true> with spmv_scs64_halo's block order, wait and gather (a halo column's float is the low half of its slot)
__global__ __launch_bounds__(256) void spmv_scs64_halo_f32(const uint32_t* __restrict__ chunkPtr,
    const uint32_t* __restrict__ chunkLens, const uint32_t* __restrict__ colInd, const float* __restrict__ val,
    const float* __restrict__ x, float* __restrict__ y, uint32_t nr, uint32_t nChunks, uint32_t perXcdI,
    float* __restrict__ dotL1, const int* __restrict__ stop, ScsHalo hh)
{
  scs64_halo_spmv<4, true>(chunkPtr, chunkLens, colInd, val, x, y, nr, nChunks, perXcdI, dotL1, stop, hh,
      [&](uint32_t col) -> float { return col >= nr ? __uint_as_float((unsigned)hh.ext[col - nr]) : x[col]; },
      xor_sum_f<64>);
}

// host transport (its neighbour_exchange carries doubles): pack widening out[i] = (double)in[idx[i]], unpack narrowing into the
// float tail -- both exact
__global__ __launch_bounds__(256) void halo_pack_wide_f32_k(uint32_t n, const uint32_t* __restrict__ idx, const float* __restrict__ in,
    double* __restrict__ out, const int* __restrict__ stop)
{
  if (stop && *stop) return;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (double)in[idx[i]];
}
__global__ __launch_bounds__(256) void halo_unpack_narrow_f32_k(uint32_t n, const double* __restrict__ in, float* __restrict__ out)
{
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (float)in[i];
}

} // namespace sbk
