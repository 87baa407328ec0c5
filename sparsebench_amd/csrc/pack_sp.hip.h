// pack_sp.hip.h -- single precision on the masked row programs (pack.hip.h level 6): the float counterparts of
// spmv_scs64_pat<CPT, DOT, SKIPPAD, false, true> and spmv_prog_fusep<CPT, SKIPPAD, false, MAPPED>, for matrices whose chunks
// are ALL row programs and whose windows are all of the mapped or of the simple kind (sb_matrix_all_row_programs): no class
// dictionary, no per-lane code words, no exception entries, no halo-waiting tiles.
//
// Nothing about the mirror's structure carries a precision: tile headers, signed row bases, slot maps, program masks and
// offsets are used as the fp64 builder made them (sbhip_sp.inc.h: the builder runs on the floats' bit patterns).  Only the
// program values and the x window are floats here: a program block is 128 bytes instead of 192, the window takes half the
// LDS, an x read is a 4-byte LDS load.  Every product is rounded to float before its add (v_mul_f32, then v_add_f32 under
// EXEC = mask; -ffp-contract=off), a row's additions run left to right as in the reference's loops, the dot's level-0
// butterflies and level-1 combine are those of spmv_scs64_f32<true> (kernels_sp.hip.h): same bits as the streaming kernels.
#pragma once
#include "kernels_sp.hip.h"
#include "pack.hip.h"

namespace sbk {

// a batch of 8 program entries stays three scalar loads: values (8 dwords), offsets (8 dwords), masks (16 dwords)
struct ProgBlockF {
  float v[8];
  uint32_t off4[8];           // byte offset of the entry's x in the float window, relative to 4 * the row's base slot
  unsigned long long mask[8]; // lanes that have the entry
};
static_assert(sizeof(ProgBlockF) == 128, "blocks stay 64-byte aligned");
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ProgBlock -> ProgBlockF (once, at upload).  The builder ran on doubles whose 64-bit pattern is the float's 32 bits
// zero-extended: the value is the pattern's low word.  off8 is 8 * (slot - base slot) as a signed 32-bit number (row bases may
// be negative; the sums wrap), so the float window's offset is half of it, taken signed.
__global__ __launch_bounds__(256) void prog_narrow_k(const ProgBlock* __restrict__ in, ProgBlockF* __restrict__ out, uint32_t nBlocks)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nBlocks * 8u) return;
  const uint32_t b = i >> 3, q = i & 7u;
  const unsigned long long bits = reinterpret_cast<const unsigned long long*>(in[b].v)[q];
  out[b].v[q]    = __uint_as_float((uint32_t)bits);
  out[b].off4[q] = (uint32_t)((int32_t)in[b].off8[q] / 2);
  out[b].mask[q] = in[b].mask[q];
}

// acc += prod in the lanes of `mask` only (masked_add's float form: same conditions on the caller)
__device__ __forceinline__ void masked_add_f(float& acc, float prod, unsigned long long mask)
{
  asm volatile("s_mov_b64 exec, %2\n\tv_add_f32 %0, %0, %1\n\ts_mov_b64 exec, -1" : "+v"(acc) : "v"(prod), "s"(mask));
}

// the first N (8 or 4) entries of a program block: entry loads (scalar), x reads (LDS, 4 bytes), then products and adds
template <int N, bool MASK>
__device__ __forceinline__ void prog_batch_f(const ProgBlockF* __restrict__ blk, uint32_t base4x, const char* ldsBytes, float& acc)
{
  float v[N], xs[N];
  unsigned long long mk[N];
  uint32_t o[N];
  if (N == 8) { // uniform addresses: s_load_dwordx8 / x8 / x16
    const f32x8 vv = *reinterpret_cast<const f32x8*>(blk->v);
    const u32x8 oo = *reinterpret_cast<const u32x8*>(blk->off4);
#pragma unroll
    for (int q = 0; q < N; q++) v[q] = vv[q], o[q] = oo[q];
    if (MASK) {
      const u64x8 mm = *reinterpret_cast<const u64x8*>(blk->mask);
#pragma unroll
      for (int q = 0; q < N; q++) mk[q] = mm[q];
    }
  } else {
    const f32x4 vv = *reinterpret_cast<const f32x4*>(blk->v);
    const u32x4 oo = *reinterpret_cast<const u32x4*>(blk->off4);
    const u64x4 mm = *reinterpret_cast<const u64x4*>(blk->mask);
#pragma unroll
    for (int q = 0; q < N; q++) v[q] = vv[q], o[q] = oo[q], mk[q] = mm[q];
  }
#pragma unroll
  for (int q = 0; q < N; q++) xs[q] = *reinterpret_cast<const float*>(ldsBytes + (base4x + o[q]));
#pragma unroll
  for (int q = 0; q < N; q++) {
    const float prod = v[q] * xs[q];
    if (MASK) masked_add_f(acc, prod, mk[q]);
    else acc = acc + prod;
  }
}

// one chunk's row program: every lane runs every entry, the adds under the entry's mask; then the reference's padding term
template <bool SKIPPAD>
__device__ __forceinline__ float run_program_f(const ProgBlockF* __restrict__ pg, uint32_t lenf, uint32_t base4x,
    const char* ldsBytes, unsigned long long padMask, float xpad)
{
  const uint32_t len = lenf & PAT_LEN_MASK;
  float acc          = 0.0f;
  uint32_t j0        = 0;
  // (not unrolled: a second batch in flight costs scalar and vector registers, i.e. occupancy -- pack.hip.h)
  if (lenf & PAT_NOPAD) { // wave-uniform: every lane has every entry
#pragma unroll 1
    for (; j0 + 8u <= len; j0 += 8u) prog_batch_f<8, false>(pg + (j0 >> 3), base4x, ldsBytes, acc);
  } else {
#pragma unroll 1
    for (; j0 + 8u <= len; j0 += 8u) prog_batch_f<8, true>(pg + (j0 >> 3), base4x, ldsBytes, acc);
  }
  if (j0 + 4u < len) prog_batch_f<8, true>(pg + (j0 >> 3), base4x, ldsBytes, acc); // 5..7 entries left (the rest: mask 0)
  else if (j0 < len) prog_batch_f<4, true>(pg + (j0 >> 3), base4x, ldsBytes, acc); // 1..4
  // src/matrix-SCS.c:151-155 / :208-227: a row shorter than its chunk adds 0.0 * x[padCol] per missing column; once is the same
  if (!SKIPPAD && (lenf & PAT_HASPAD)) masked_add_f(acc, 0.0f * xpad, padMask);
  return acc;
}

// y = A x over the row programs.  CPT: chunks per tile (4 or 8: a wave multiplies one or two chunks behind one header fetch,
// one window staging and one barrier); DOT: the tile's level-1 values of x . y; SKIPPAD: the CRS format's mirror (no padding
// terms); MAPPED: the window is laid out in original column order and staged through the 16-bit slot map (sigma > 1), else
// segment by segment (simple windows: three segments of <= 256 * LONG entries and three of <= 256).
// Window columns >= nr are read from the tail of x (several ranks: the halo exchange has filled it before the launch).
template <int CPT, bool DOT, bool SKIPPAD, bool MAPPED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(72))) void spmv_prog_f32(const uint32_t* __restrict__ hdrWords,
    const int16_t* __restrict__ rowBase, const ProgBlockF* __restrict__ progs, const uint16_t* __restrict__ slotMap,
    uint32_t mapStride, const float* __restrict__ x, float* __restrict__ y, uint32_t nr, uint32_t nChunks, uint32_t nHdrs,
    uint32_t blocksPerXcd, uint32_t padCol, float* __restrict__ dotL1, const int* __restrict__ stop)
{
  extern __shared__ __attribute__((aligned(16))) float ldsF[]; // [16 floats: level-1 combine][window]
  float* sq = ldsF;
  float* sx = ldsF + 16;
  constexpr int CW   = CPT / 4;          // chunks per wave
  constexpr int LONG = CPT == 8 ? 4 : 3; // loads per thread for each of the three long segments of a simple window
  constexpr int WB   = 3 * LONG + 3;     // window entries per thread
  const uint32_t tile0 = xcd_block(blockIdx.x, blocksPerXcd);
  const uint32_t hidx  = min(tile0, nHdrs - 1u); // clamped: every load below is unconditional
  // round trip 1: ONE vector load brings the tile header (lanes 0..47) and the stop flag (lane 48)
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t hvx, hvy = 0u;
  if (CPT == 4) {
    const uint32_t* hp = hdrWords + (size_t)hidx * 48u;
    hvx = *(lane < (uint32_t)PAT_STOP_LANE ? hp + lane : reinterpret_cast<const uint32_t*>(stop));
  } else {
    const u32x2* hp = reinterpret_cast<const u32x2*>(hdrWords + (size_t)hidx * 128u);
    const u32x2 h2  = *(lane < (uint32_t)PAT_STOP_LANE ? hp + lane : reinterpret_cast<const u32x2*>(stop));
    hvx = h2.x, hvy = h2.y;
  }
  uint32_t dmap[MAPPED ? WB : 1];
  if (MAPPED) { // (distinct maps stored once behind a header -> map table: sbhip_matrix.inc.h)
    const uint32_t mStr = mapStride & 0xFFFu, mOff = (mapStride >> 12) * 256u;
    const uint32_t mIdx = mOff ? reinterpret_cast<const uint32_t*>(slotMap)[hidx] : hidx;
    const uint16_t* mp  = slotMap + mOff + (size_t)mIdx * mStr + threadIdx.x;
#pragma unroll
    for (int k = 0; k < WB; k++) dmap[k] = mp[min((uint32_t)k * 256u, mStr - 256u)];
  }
  auto field = [&](int i) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)hvx, i); };
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  auto cfield = [&](int c, int i) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)(c == 0 ? hvx : hvy), i); };
  const int stopped   = (int)field(PAT_STOP_LANE);
  const uint32_t tile = field(46), win = field(3);
  // round trip 2: row bases, own x entries, x window -- addresses clamped into valid memory so that nothing waits for a branch
  uint32_t chunk[CW], row[CW], lenf[CW];
  int32_t base[CW];
  float xrow[CW];
#pragma unroll
  for (int c = 0; c < CW; c++) {
    chunk[c] = tile * CPT + wv + 4u * (uint32_t)c;
    row[c]   = chunk[c] * 64u + lane;
    lenf[c]  = cfield(c, 8 + (int)wv);
    base[c]  = (int32_t)rowBase[chunk[c] < nChunks ? row[c] : 0u];
    xrow[c]  = DOT ? x[min(row[c], nr - 1u)] : 0.0f;
  }
  const float xpad = x[padCol]; // slot 0: what padding multiplies
  float t[WB];
  if (MAPPED) { // slot by slot through the map (the 18 segment words hold the base column of every 256 slots)
#pragma unroll
    for (int k = 0; k < WB; k++) t[k] = x[field(12 + min(k, 17)) + dmap[MAPPED ? k : 0]];
  } else { // segment by segment: entry i of segment s -> slot first_s + i
#pragma unroll
    for (int sI = 0; sI < 3; sI++) {
      const uint32_t sc = field(12 + 3 * sI), sn = field(12 + 3 * sI + 2);
#pragma unroll
      for (int r = 0; r < LONG; r++) t[sI * LONG + r] = x[sn ? sc + min((uint32_t)r * 256u + threadIdx.x, sn - 1u) : padCol];
    }
#pragma unroll
    for (int sI = 3; sI < 6; sI++) {
      const uint32_t sc = field(12 + 3 * sI), sn = field(12 + 3 * sI + 2);
      t[3 * LONG + sI - 3] = x[sn ? sc + min(threadIdx.x, sn - 1u) : padCol];
    }
  }
  // keep every load above in front of the exit test (the compiler would sink them behind it)
#pragma unroll
  for (int k = 0; k < WB; k++) asm volatile("" ::"v"(t[k]));
#pragma unroll
  for (int c = 0; c < CW; c++) asm volatile("" ::"v"(base[c]), "v"(xrow[c]));
  asm volatile("" ::"v"(xpad));
  if (tile0 >= nHdrs || stopped) return; // uniform per workgroup
  if (MAPPED) {
#pragma unroll
    for (int k = 0; k < WB; k++) {
      const uint32_t slot = (uint32_t)k * 256u + threadIdx.x;
      if (slot < win) sx[slot] = t[k]; // (the host builds no window beyond 256 * WB slots: sbhip_sp.inc.h checks)
    }
    if (threadIdx.x == 0) sx[0] = xpad;
  } else {
    if (threadIdx.x == 0) sx[0] = xpad;
#pragma unroll
    for (int sI = 0; sI < 3; sI++) {
      const uint32_t sf = field(12 + 3 * sI + 1), sn = field(12 + 3 * sI + 2);
#pragma unroll
      for (int r = 0; r < LONG; r++) {
        const uint32_t i = (uint32_t)r * 256u + threadIdx.x;
        if (i < sn) sx[sf + i] = t[sI * LONG + r];
      }
    }
#pragma unroll
    for (int sI = 3; sI < 6; sI++) {
      const uint32_t sf = field(12 + 3 * sI + 1), sn = field(12 + 3 * sI + 2);
      if (threadIdx.x < sn) sx[sf + threadIdx.x] = t[3 * LONG + sI - 3];
    }
  }
  __syncthreads();
  constexpr uint32_t sxOff = 16u * (uint32_t)sizeof(float);
  const char* ldsBytes     = reinterpret_cast<const char*>(ldsF);
  float pl0[CW]; // (DOT) the wave's level-0 partials of x . y; +0.0 for chunks past the end
#pragma unroll
  for (int c = 0; c < CW; c++) pl0[c] = 0.0f;
#pragma unroll
  for (int c = 0; c < CW; c++) {
    if (chunk[c] >= nChunks) continue; // wave-uniform; inactive waves only helped staging
    const unsigned long long padMask =
        (unsigned long long)cfield(c, 36 + 2 * (int)wv) | ((unsigned long long)cfield(c, 37 + 2 * (int)wv) << 32);
    const float acc = run_program_f<SKIPPAD>(progs + cfield(c, 32 + (int)wv), lenf[c], ((uint32_t)base[c] << 2) + sxOff, ldsBytes,
        padMask, xpad);
    if (row[c] < nr) y[row[c]] = acc;
    if (DOT) pl0[c] = xor_sum_f<64>(row[c] < nr ? xrow[c] * acc : 0.0f);
  }
  // the tile's LEVEL-1 values ((q0 + q1) + q2) + q3 of its aligned groups of four chunks, behind ONE barrier: exactly what
  // spmv_scs64_f32<true> writes
  if (DOT) {
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < CW; c++) sq[wv + 4u * (uint32_t)c] = pl0[c];
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)CW) {
      const uint32_t gq = threadIdx.x, group = tile * (uint32_t)CW + gq;
      if (group < ((nChunks + 3u) >> 2)) dotL1[group] = ((sq[4u * gq] + sq[4u * gq + 1u]) + sq[4u * gq + 2u]) + sq[4u * gq + 3u];
    }
  }
}

// =============================================================================
// SpMV of the SP CG loop WITH the p update inside (spmv_prog_fusep's float counterpart, one rank): Ap = A p_new with
// p_new = r + beta p_old formed while the window is staged (src/CGSolver.c:114 and :123; which != 0, the first body:
// p_new = r + 0.0f * r, :109, the host passes pold = r), p_new and the owed x += alpha p_old (:127) stored for the tile's own
// rows, the level-1 values of p_new . Ap.  p is double-buffered (other tiles still read p_old).  Element for element the
// arithmetic of cg_update_p_f32 followed by the row programs: same bits as the two kernels it replaces.
// The window is staged in TWO passes of <= 8 slots per thread, each loading p_old AND r: one dependent round trip more per
// tile instead of 14 more live registers (<= 64 VGPRs: 8 workgroups per CU).
// =============================================================================
template <int CPT, bool SKIPPAD, bool MAPPED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(72))) void spmv_prog_fusep_f32(const uint32_t* __restrict__ hdrWords,
    const int16_t* __restrict__ rowBase, const ProgBlockF* __restrict__ progs, const uint16_t* __restrict__ slotMap,
    uint32_t mapStride, const float* __restrict__ pold, const float* __restrict__ r, float* __restrict__ pnew, float* xsol,
    float* __restrict__ y, const CgScalarsF* __restrict__ S, int which, uint32_t nr, uint32_t nChunks, uint32_t nHdrs,
    uint32_t blocksPerXcd, uint32_t padCol, float* __restrict__ dotL1)
{
  extern __shared__ __attribute__((aligned(16))) float ldsF[]; // [16 floats: level-1 combine][window]
  float* sq = ldsF;
  float* sx = ldsF + 16;
  constexpr int CW   = CPT / 4;
  constexpr int LONG = CPT == 8 ? 4 : 3;
  constexpr int WB   = 3 * LONG + 3;
  constexpr int H1   = 8; // slots per thread in the first pass (loaded in front of the exit test)
  const uint32_t tile0 = xcd_block(blockIdx.x, blocksPerXcd);
  const uint32_t hidx  = min(tile0, nHdrs - 1u);
  const uint32_t lane  = threadIdx.x & 63u;
  uint32_t hvx, hvy = 0u;
  // (CgScalarsF: `stop` sits at byte 32, 8-byte aligned, stop_next behind it: the 8-byte load of the 8-chunk header works)
  if (CPT == 4) {
    const uint32_t* hp = hdrWords + (size_t)hidx * 48u;
    hvx = *(lane < (uint32_t)PAT_STOP_LANE ? hp + lane : reinterpret_cast<const uint32_t*>(&S->stop));
  } else {
    const u32x2* hp = reinterpret_cast<const u32x2*>(hdrWords + (size_t)hidx * 128u);
    const u32x2 h2  = *(lane < (uint32_t)PAT_STOP_LANE ? hp + lane : reinterpret_cast<const u32x2*>(&S->stop));
    hvx = h2.x, hvy = h2.y;
  }
  // (mapped windows) the second pass's map entries ride in the high halves of the first pass's registers
  uint32_t dmap[MAPPED ? H1 : 1];
  if (MAPPED) {
    const uint32_t mStr = mapStride & 0xFFFu, mOff = (mapStride >> 12) * 256u;
    const uint32_t mIdx = mOff ? reinterpret_cast<const uint32_t*>(slotMap)[hidx] : hidx;
    const uint16_t* mp  = slotMap + mOff + (size_t)mIdx * mStr + threadIdx.x;
    uint32_t lo[H1], hi[H1];
#pragma unroll
    for (int k = 0; k < H1; k++) {
      lo[k] = mp[min((uint32_t)k * 256u, mStr - 256u)];
      hi[k] = k + H1 < WB ? (uint32_t)mp[min((uint32_t)(k + H1) * 256u, mStr - 256u)] : 0u;
    }
#pragma unroll
    for (int k = 0; k < H1; k++) dmap[k] = lo[k] | (hi[k] << 16);
  }
  // the step's scalars (uniform: scalar loads, back with the header)
  const float beta  = which ? 0.0f : (float)S->beta; // cg_update_p_f32: the float value the reference's `double beta` carries
  const float alpha = S->alpha;
  const bool owed   = !which && S->x_pending != 0;
  auto field = [&](int i) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)hvx, i); };
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  auto cfield = [&](int c, int i) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)(c == 0 ? hvx : hvy), i); };
  const int stopped   = (int)field(PAT_STOP_LANE);
  const uint32_t tile = field(46), win = field(3);
  auto col_of = [&](int k) -> uint32_t { // which column slot k of this thread holds
    if (MAPPED) return field(12 + min(k, 17)) + (k < H1 ? dmap[MAPPED ? k : 0] & 0xFFFFu : dmap[MAPPED ? k - H1 : 0] >> 16);
    const int sI = k < 3 * LONG ? k / LONG : 3 + (k - 3 * LONG);
    const uint32_t i = (k < 3 * LONG ? (uint32_t)(k % LONG) * 256u : 0u) + threadIdx.x;
    const uint32_t sc = field(12 + 3 * sI), sn = field(12 + 3 * sI + 2);
    return sn ? sc + min(i, sn - 1u) : padCol;
  };
  auto slot_of = [&](int k, bool& valid) -> uint32_t { // where it goes, whether it exists
    if (MAPPED) {
      const uint32_t slot = (uint32_t)k * 256u + threadIdx.x;
      valid = slot < win;
      return slot;
    }
    const int sI = k < 3 * LONG ? k / LONG : 3 + (k - 3 * LONG);
    const uint32_t i = (k < 3 * LONG ? (uint32_t)(k % LONG) * 256u : 0u) + threadIdx.x;
    valid = i < field(12 + 3 * sI + 2);
    return field(12 + 3 * sI + 1) + i;
  };
  float pv[H1], rv[H1];
#pragma unroll
  for (int k = 0; k < H1; k++) {
    const uint32_t c = col_of(k);
    pv[k] = pold[c], rv[k] = r[c];
  }
  uint32_t chunk[CW], row[CW], lenf[CW];
  int32_t base[CW];
#pragma unroll
  for (int c = 0; c < CW; c++) {
    chunk[c] = tile * CPT + wv + 4u * (uint32_t)c;
    row[c]   = chunk[c] * 64u + lane;
    lenf[c]  = cfield(c, 8 + (int)wv);
    base[c]  = (int32_t)rowBase[chunk[c] < nChunks ? row[c] : 0u];
  }
#pragma unroll
  for (int k = 0; k < H1; k++) asm volatile("" ::"v"(pv[k]), "v"(rv[k]));
#pragma unroll
  for (int c = 0; c < CW; c++) asm volatile("" ::"v"(base[c]));
  if (tile0 >= nHdrs || stopped) return; // uniform per workgroup
  // slot 0: what padding multiplies, p_new[padCol] (uniform addresses: scalar loads)
  const float xpad = r[padCol] + beta * pold[padCol];
  if (!MAPPED && threadIdx.x == 0) sx[0] = xpad;
#pragma unroll
  for (int k = 0; k < H1; k++) {
    bool valid;
    const uint32_t slot = slot_of(k, valid);
    const float pn      = rv[k] + beta * pv[k];
    if (valid) sx[slot] = pn;
  }
  { // second pass: the same registers again
    float pw[WB - H1], rw[WB - H1];
#pragma unroll
    for (int k = H1; k < WB; k++) {
      const uint32_t c = col_of(k);
      pw[k - H1] = pold[c], rw[k - H1] = r[c];
    }
#pragma unroll
    for (int k = H1; k < WB; k++) {
      bool valid;
      const uint32_t slot = slot_of(k, valid);
      const float pn      = rw[k - H1] + beta * pw[k - H1];
      if (valid) sx[slot] = pn;
    }
  }
  if (MAPPED && threadIdx.x == 0) sx[0] = xpad; // (behind this thread's own store to slot 0)
  __syncthreads();
  // own rows: p_old, r and (if the previous body owes it) x, behind the barrier so that their latency hides behind the programs
  float rown[CW], xown[CW], prow[CW];
#pragma unroll
  for (int c = 0; c < CW; c++) {
    const uint32_t rr = min(row[c], nr - 1u);
    prow[c] = pold[rr];
    rown[c] = r[rr];
    xown[c] = owed ? xsol[rr] : 0.0f;
  }
  constexpr uint32_t sxOff = 16u * (uint32_t)sizeof(float);
  const char* ldsBytes     = reinterpret_cast<const char*>(ldsF);
  float pl0[CW];
#pragma unroll
  for (int c = 0; c < CW; c++) pl0[c] = 0.0f;
#pragma unroll
  for (int c = 0; c < CW; c++) {
    if (chunk[c] >= nChunks) continue; // wave-uniform
    const unsigned long long padMask =
        (unsigned long long)cfield(c, 36 + 2 * (int)wv) | ((unsigned long long)cfield(c, 37 + 2 * (int)wv) << 32);
    const float acc = run_program_f<SKIPPAD>(progs + cfield(c, 32 + (int)wv), lenf[c], ((uint32_t)base[c] << 2) + sxOff, ldsBytes,
        padMask, xpad);
    float t2 = 0.0f;
    if (row[c] < nr) {
      y[row[c]] = acc;
      const float po = prow[c], pn = rown[c] + beta * po; // cg_update_p_f32's arithmetic for the own row
      pnew[row[c]] = pn;
      if (owed) xsol[row[c]] = xown[c] + alpha * po;
      t2 = pn * acc;
    }
    pl0[c] = xor_sum_f<64>(t2);
  }
  // the tile's level-1 values of p_new . Ap (as spmv_prog_f32<..., DOT> forms them)
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < CW; c++) sq[wv + 4u * (uint32_t)c] = pl0[c];
  }
  __syncthreads();
  if (threadIdx.x < (uint32_t)CW) {
    const uint32_t gq = threadIdx.x, group = tile * (uint32_t)CW + gq;
    if (group < ((nChunks + 3u) >> 2)) dotL1[group] = ((sq[4u * gq] + sq[4u * gq + 1u]) + sq[4u * gq + 2u]) + sq[4u * gq + 3u];
  }
}

// the owed x += alpha p of the LAST body that ran, with p double-buffered: body k leaves p_k in buffer k & 1 and n_pAp bodies
// have run (cg_x_finalize's float form)
__global__ __launch_bounds__(256) void cg_x_finalize2_f32(uint32_t n, float* x, const float* __restrict__ p0,
    const float* __restrict__ p1, const CgScalarsF* __restrict__ S)
{
  if (!S->x_pending) return;
  const float* __restrict__ p = (S->n_pAp & 1) ? p1 : p0;
  const float alpha     = S->alpha;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] = x[i] + alpha * p[i];
}

} // namespace sbk
