// sbhip_sgs.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): the symmetric
// Gauss-Seidel preconditioner of PCG by multicolouring (kernels: sgs.hip.h).  The handle is an sb_pcg whose `sgs`
// plan is set: the loop, its control block, histories and every other sb_pcg_* call are sbhip_pcg.inc.h's; what differs is how
// z is made (the r update without z, nC forward launches, nC - 1 backward launches, r.z by dot_l1_k).
// ===========================================================================
// multicolour symmetric Gauss-Seidel
// ===========================================================================
struct SgsPlan {
  uint32_t nC = 0, nChunks = 0;
  std::vector<uint32_t> chunk0;  // nC + 1: first chunk of every colour
  std::vector<uint32_t> colour;  // device row order
  uint32_t* rowIdx = nullptr;    // device, nChunks * 64
  SgsHalf half[2];               // [0] lower / forward, [1] upper / backward; device arrays
  double* t = nullptr;           // the forward sums
  double *ar = nullptr, *at = nullptr, *az = nullptr; // sb_pcg_apply_precond's scratch vectors (first call)
  double structBytes = 0.0;      // the sweep structure as one apply reads it
  double halfBytes[2] = { 0.0, 0.0 }; // each half over all its chunks (a sweep from a guess reads both: sbhip_mg.inc.h)
  uint32_t rowsBackward = 0;     // rows of the colours 0 .. nC - 2
};

namespace {
// the matrix in device numbering as rows of (col, val) in storage order, entry for entry as stored (padding included)
struct HostRows {
  std::vector<size_t> ptr;
  std::vector<uint32_t> col;
  std::vector<double> val;
};
HostRows sgs_download(const sb_matrix* m)
{
  HostRows h;
  const uint32_t nr = m->nr;
  h.ptr.assign((size_t)nr + 1, 0);
  if (nr == 0) return h;
  if (m->fmt == 0) {
    std::vector<uint32_t> rp((size_t)nr + 1);
    sb_d2h(rp.data(), m->rowPtr, rp.size() * sizeof(uint32_t));
    const size_t nnz = rp[nr];
    h.col.resize(nnz), h.val.resize(nnz);
    if (nnz) sb_d2h(h.col.data(), m->colInd, nnz * sizeof(uint32_t)), sb_d2h(h.val.data(), m->val, nnz * sizeof(double));
    for (uint32_t i = 0; i <= nr; i++) h.ptr[i] = rp[i];
    return h;
  }
  std::vector<uint32_t> cp(m->nChunks), cl(m->nChunks), col(m->nElems);
  std::vector<double> val(m->nElems);
  sb_d2h(cp.data(), m->chunkPtr, cp.size() * sizeof(uint32_t)), sb_d2h(cl.data(), m->chunkLens, cl.size() * sizeof(uint32_t));
  if (m->nElems) sb_d2h(col.data(), m->colInd, col.size() * sizeof(uint32_t)), sb_d2h(val.data(), m->val, val.size() * sizeof(double));
  const uint32_t C = m->C;
  for (uint32_t i = 0; i < nr; i++) h.ptr[i + 1] = h.ptr[i] + cl[i / C];
  h.col.resize(h.ptr[nr]), h.val.resize(h.ptr[nr]);
  for (uint32_t i = 0; i < nr; i++) {
    const uint32_t chunk = i / C, k = i - chunk * C;
    size_t o             = h.ptr[i];
    for (uint32_t j = 0; j < cl[chunk]; j++, o++) {
      const size_t idx = (size_t)cp[chunk] + (size_t)j * C + k;
      h.col[o] = col[idx], h.val[o] = val[idx];
    }
  }
  return h;
}
template <class T> T* sgs_to_device(const std::vector<T>& v)
{
  T* d = (T*)sb_malloc(v.size() * sizeof(T));
  if (!v.empty()) sb_h2d(d, v.data(), v.size() * sizeof(T));
  return d;
}
} // namespace

// kept lists, symmetrised adjacency, greedy colouring in device row order, the two halves as Sell-64 per colour; h: the
// matrix's rows as sgs_download gives them (a caller that has downloaded them for its own use passes them on); who: the entry
// point, and the level where there are several, as messages name them
static SgsPlan* sgs_build(const sb_matrix* m, HostRows h, const char* who)
{
  SgsPlan* P        = new SgsPlan();
  const uint32_t nr = m->nr;
  // kept entries: col != row and val != 0.0 (Sell padding is a stored +0.0 and drops out by the same rule); compacted in place
  {
    size_t o = 0;
    for (uint32_t i = 0; i < nr; i++) {
      const size_t b = h.ptr[i], e = h.ptr[i + 1];
      h.ptr[i]       = o;
      for (size_t q = b; q < e; q++)
        if (h.col[q] != i && h.val[q] != 0.0) {
          if (h.col[q] >= nr) SB_FATAL("%s: device row %u has column %u outside the %u rows", who, i, h.col[q], nr);
          h.col[o] = h.col[q], h.val[o] = h.val[q], o++;
        }
    }
    h.ptr[nr] = o;
    h.col.resize(o), h.val.resize(o);
  }
  // the transposed pattern: rows j with a kept a_ji
  std::vector<size_t> tptr((size_t)nr + 1, 0);
  for (uint32_t c : h.col) tptr[(size_t)c + 1]++;
  for (uint32_t i = 0; i < nr; i++) tptr[i + 1] += tptr[i];
  std::vector<uint32_t> tcol(h.col.size());
  {
    std::vector<size_t> fill(tptr.begin(), tptr.end() - 1);
    for (uint32_t i = 0; i < nr; i++)
      for (size_t q = h.ptr[i]; q < h.ptr[i + 1]; q++) tcol[fill[h.col[q]]++] = i;
  }
  // rows 0, 1, ... each take the smallest colour no adjacent, already coloured row has
  P->colour.assign(nr, 0);
  std::vector<uint32_t> seen; // seen[c] == i + 1: colour c is taken around row i
  for (uint32_t i = 0; i < nr; i++) {
    auto mark = [&](uint32_t j) {
      if (j >= i) return;
      const uint32_t c = P->colour[j];
      if (c >= seen.size()) seen.resize((size_t)c + 1, 0);
      seen[c] = i + 1;
    };
    for (size_t q = h.ptr[i]; q < h.ptr[i + 1]; q++) mark(h.col[q]);
    for (size_t q = tptr[i]; q < tptr[i + 1]; q++) mark(tcol[q]);
    uint32_t c = 0;
    while (c < seen.size() && seen[c] == i + 1) c++;
    P->colour[i] = c;
    if (c + 1 > P->nC) P->nC = c + 1;
  }
  // chunks: the rows of a colour ascending, 64 to a chunk
  const uint32_t nC = P->nC;
  std::vector<uint32_t> count(nC, 0);
  for (uint32_t i = 0; i < nr; i++) count[P->colour[i]]++;
  P->chunk0.assign((size_t)nC + 1, 0);
  for (uint32_t c = 0; c < nC; c++) P->chunk0[c + 1] = P->chunk0[c] + (count[c] + 63u) / 64u;
  P->nChunks      = nC ? P->chunk0[nC] : 0;
  P->rowsBackward = nC ? nr - count[nC - 1] : 0;
  std::vector<uint32_t> rowIdx((size_t)P->nChunks * 64u, 0xFFFFFFFFu);
  {
    std::vector<size_t> next(nC);
    for (uint32_t c = 0; c < nC; c++) next[c] = (size_t)P->chunk0[c] * 64u;
    for (uint32_t i = 0; i < nr; i++) rowIdx[next[P->colour[i]]++] = i;
  }
  P->rowIdx = sgs_to_device(rowIdx);
  // the halves: lower(i) the kept entries whose column's colour is less than colour(i), upper(i) those with a greater one, each
  // in storage order, column-major per chunk; padding is (+0.0, column 0) and is never used (the lane's own length stops it)
  for (int up = 0; up < 2; up++) {
    auto in_half = [&](uint32_t i, size_t q) {
      const uint32_t ci = P->colour[i], cj = P->colour[h.col[q]];
      if (ci == cj) SB_FATAL("%s: device rows %u and %u are adjacent and share colour %u", who, i, h.col[q], ci);
      return up ? cj > ci : cj < ci;
    };
    std::vector<uint32_t> rowLen(rowIdx.size(), 0), chunkLen(P->nChunks, 0);
    std::vector<unsigned long long> chunkPtr((size_t)P->nChunks + 1, 0);
    for (size_t sl = 0; sl < rowIdx.size(); sl++) {
      const uint32_t i = rowIdx[sl];
      if (i == 0xFFFFFFFFu) continue;
      uint32_t len = 0;
      for (size_t q = h.ptr[i]; q < h.ptr[i + 1]; q++) len += in_half(i, q) ? 1u : 0u;
      rowLen[sl]       = len;
      chunkLen[sl / 64] = std::max(chunkLen[sl / 64], len);
    }
    for (uint32_t c = 0; c < P->nChunks; c++) chunkPtr[c + 1] = chunkPtr[c] + (unsigned long long)chunkLen[c] * 64u;
    std::vector<uint32_t> col(chunkPtr[P->nChunks], 0);
    std::vector<double> val(chunkPtr[P->nChunks], 0.0);
    for (size_t sl = 0; sl < rowIdx.size(); sl++) {
      const uint32_t i = rowIdx[sl];
      if (i == 0xFFFFFFFFu) continue;
      size_t o = chunkPtr[sl / 64] + (sl & 63u);
      for (size_t q = h.ptr[i]; q < h.ptr[i + 1]; q++)
        if (in_half(i, q)) col[o] = h.col[q], val[o] = h.val[q], o += 64;
    }
    SgsHalf& H = P->half[up];
    H.chunkPtr = sgs_to_device(chunkPtr), H.chunkLen = sgs_to_device(chunkLen), H.rowLen = sgs_to_device(rowLen);
    H.col = sgs_to_device(col), H.val = sgs_to_device(val);
    // what one apply reads of it: the backward sweep leaves the last colour's chunks alone
    const uint32_t chunksRead = up ? (nC ? P->chunk0[nC - 1] : 0) : P->nChunks;
    P->structBytes += (double)chunkPtr[chunksRead] * 12.0 + (double)chunksRead * (64.0 * 8.0 + 12.0); // val + col | rowIdx, rowLen, chunkPtr, chunkLen
    P->halfBytes[up] = (double)chunkPtr[P->nChunks] * 12.0 + (double)P->nChunks * (64.0 * 8.0 + 12.0);
  }
  P->t = (double*)sb_malloc((size_t)nr * sizeof(double) + 4096);
  return P;
}
static SgsPlan* sgs_build(const sb_matrix* m) { return sgs_build(m, sgs_download(m), "sb_pcg_create_sgs"); }

static void sgs_free_plan(SgsPlan* P)
{
  if (!P) return;
  sb_free(P->rowIdx), sb_free(P->t), sb_free(P->ar), sb_free(P->at), sb_free(P->az);
  for (SgsHalf& H : P->half)
    sb_free((void*)H.chunkPtr), sb_free((void*)H.chunkLen), sb_free((void*)H.rowLen), sb_free((void*)H.col), sb_free((void*)H.val);
  delete P;
}
static void sgs_release(sb_pcg* s)
{
  sgs_free_plan(s->sgs);
  s->sgs = nullptr;
}

// z = M^-1 r: forward over the colours 0 .. nC-1, backward over nC-2 .. 0; one launch per colour (a wave per chunk)
static dim3 sgs_grid(const SgsPlan* P, uint32_t c) { return dim3((P->chunk0[c + 1] - P->chunk0[c] + 3u) / 4u); }
// the backward sweep alone: from the forward sums in t
static void sgs_backward(const SgsPlan* P, const double* dinv, double* t, double* z, const int* stop)
{
  for (uint32_t c = P->nC > 1 ? P->nC - 1 : 0; c-- > 0;)
    hipLaunchKernelGGL(sgs_sweep_k<1>, sgs_grid(P, c), dim3(256), 0, g.stream, P->chunk0[c], P->chunk0[c + 1] - P->chunk0[c],
        (const uint32_t*)P->rowIdx, P->half[1], (const double*)t, dinv, t, z, stop);
}
static void sgs_apply(const SgsPlan* P, const double* dinv, const double* r, double* t, double* z, const int* stop)
{
  for (uint32_t c = 0; c < P->nC; c++)
    hipLaunchKernelGGL(sgs_sweep_k<0>, sgs_grid(P, c), dim3(256), 0, g.stream, P->chunk0[c], P->chunk0[c + 1] - P->chunk0[c],
        (const uint32_t*)P->rowIdx, P->half[0], r, dinv, t, z, stop);
  sgs_backward(P, dinv, t, z, stop);
  HIP_CHECK(hipGetLastError());
}
// the handle's preconditioner: the sweeps of its matrix, or the V-cycle around them
static void sgs_apply(const sb_pcg* s, const double* r, double* t, double* z, const int* stop)
{
  if (s->mg) mg_apply(s, r, t, z, stop);
  else sgs_apply(s->sgs, (const double*)s->dinv, r, t, z, stop);
}

// the r update (PRO 1: the prologue's b - Ap) with the r.r values, the apply, the r.z values
template <int PRO> static void sgs_residual_and_z(sb_pcg* s)
{
  const uint32_t n = s->nr;
  if (!n) return;
  const int* stop = &s->S->stop; // (0 throughout the prologue: sb_pcg_start has just written the block)
  hipLaunchKernelGGL(sgs_update_r_k<PRO>, dim3(vec_stream_grid(n)), dim3(1024), 0, g.stream, n, (const double*)s->Ap,
      (const double*)(PRO ? s->b : s->r), s->r, (const PcgScalars*)s->S, s->l1rr);
  sgs_apply(s, s->r, s->sgs->t, s->z, stop);
  hipLaunchKernelGGL(dot_l1_k, dim3(vec_stream_grid(n)), dim3(1024), 0, g.stream, n, (const double*)s->r, (const double*)s->z, s->l1rz,
      stop);
  HIP_CHECK(hipGetLastError());
}
static void sgs_residual_and_z(sb_pcg* s, bool prologue) { prologue ? sgs_residual_and_z<1>(s) : sgs_residual_and_z<0>(s); }

sb_pcg* sb_pcg_create_sgs(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host)
{
  sb_pcg* s = pcg_create(m, halo, b_host, xexact_host, nullptr, "sb_pcg_create_sgs", "SGS");
  s->sgs    = sgs_build(m);
  HIP_CHECK(hipStreamSynchronize(g.stream));
  return s;
}

static bool mg_is_fw(const sb_pcg* s); // (sbhip_mg.inc.h)
int sb_pcg_precond(const sb_pcg* s) { return s->mg ? (mg_is_fw(s) ? 3 : 2) : s->sgs ? 1 : 0; }
int sb_pcg_colours(const sb_pcg* s) { return s->sgs ? (int)s->sgs->nC : 0; }

void sb_pcg_colouring(const sb_pcg* s, uint32_t* colour_host)
{
  need_init();
  if (!s->sgs) SB_FATAL("sb_pcg_colouring: the handle has a diagonal preconditioner (sb_pcg_create_sgs makes the coloured one)");
  const sb_matrix* m = s->A;
  if (m->fmt == 1 && m->permuted) {
    std::vector<uint32_t> o2n(m->nr);
    if (m->nr) sb_d2h(o2n.data(), m->oldToNew, (size_t)m->nr * sizeof(uint32_t));
    for (uint32_t i = 0; i < m->nr; i++) colour_host[i] = s->sgs->colour[o2n[i]];
  } else {
    std::copy(s->sgs->colour.begin(), s->sgs->colour.end(), colour_host);
  }
}

void sb_pcg_apply_precond(sb_pcg* s, const double* r_host, double* z_host)
{
  need_init();
  if (s->clock.open) SB_FATAL("sb_pcg_apply_precond between sb_pcg_start and sb_pcg_finish: the solve's vectors are in flight");
  const uint32_t n = s->nr;
  if (!n) return;
  const size_t nb = (size_t)n * sizeof(double) + 4096;
  if (s->sgs) {
    SgsPlan* P = s->sgs;
    if (!P->ar) P->ar = (double*)sb_malloc(nb), P->at = (double*)sb_malloc(nb), P->az = (double*)sb_malloc(nb);
    upload_permuted(s->A, r_host, P->ar);
    sgs_apply(s, P->ar, P->at, P->az, zero_flag());
    HIP_CHECK(hipStreamSynchronize(g.stream));
    download_original(s->A, P->az, z_host);
  } else {
    double *ar = (double*)sb_malloc(nb), *az = (double*)sb_malloc(nb);
    upload_permuted(s->A, r_host, ar);
    hipLaunchKernelGGL(precond_diag_k, dim3(stream_grid(n, 256)), dim3(256), 0, g.stream, n, (const double*)ar, (const double*)s->dinv, az);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(g.stream));
    download_original(s->A, az, z_host);
    sb_free(ar), sb_free(az);
  }
}

// GPU milliseconds of one apply, the mean over `reps` back-to-back applies on the scratch vectors (r = b); for the rate tool
double sb_pcg_apply_precond_ms(sb_pcg* s, int reps)
{
  need_init();
  if (s->clock.open) SB_FATAL("sb_pcg_apply_precond_ms between sb_pcg_start and sb_pcg_finish: the solve's vectors are in flight");
  const uint32_t n = s->nr;
  if (!n || reps < 1) return 0.0;
  const size_t nb = (size_t)n * sizeof(double) + 4096;
  double *ar = (double*)sb_malloc(nb), *at = (double*)sb_malloc(nb), *az = (double*)sb_malloc(nb);
  sb_d2d(ar, s->b, (size_t)n * sizeof(double));
  LoopClock c;
  c.create();
  for (int i = -1; i < reps; i++) { // (i = -1: an untimed first apply)
    if (i == 0) c.begin();
    if (s->sgs) sgs_apply(s, ar, at, az, zero_flag());
    else
      hipLaunchKernelGGL(precond_diag_k, dim3(stream_grid(n, 256)), dim3(256), 0, g.stream, n, (const double*)ar, (const double*)s->dinv, az);
  }
  c.end();
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(g.stream));
  c.read();
  c.destroy();
  sb_free(ar), sb_free(at), sb_free(az);
  return (double)c.ms / reps;
}

// bytes one apply reads and writes.  Diagonal: r, dinv in, z out.  SGS: the sweep structure, and per row forward r, dinv, one
// gathered z in, t, z out; backward (the rows of every colour but the last) t, dinv, one gathered z in, z out.  MG: mg_bytes
static double sgs_bytes(const SgsPlan* P, uint32_t nr) { return P->structBytes + 40.0 * (double)nr + 32.0 * (double)P->rowsBackward; }
static double mg_bytes(const sb_pcg* s);
double sb_pcg_precond_bytes(const sb_pcg* s)
{
  if (!s->sgs) return 24.0 * (double)s->nr;
  return s->mg ? mg_bytes(s) : sgs_bytes(s->sgs, s->nr);
}
