// sbhip_sgs.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): the symmetric
// Gauss-Seidel smoother of PCG's preconditioners by multicolouring (kernels: sgs.hip.h, mg.hip.h): its plan for one
// matrix, and its sweeps from zero and from a guess.  Which handle runs them, on which levels, is sbhip_mg.inc.h's.
// The host's one packer of Sell-64 gather structures (sell64_pack) lives here with its first user.
// ===========================================================================
// multicolour symmetric Gauss-Seidel
// ===========================================================================
struct SgsPlan {
  uint32_t nC = 0, nChunks = 0;
  std::vector<uint32_t> chunk0;  // nC + 1: first chunk of every colour
  std::vector<uint32_t> colour;  // device row order
  uint32_t* rowIdx = nullptr;    // device, nChunks * 64
  SellRows half[2];              // [0] lower / forward, [1] upper / backward; device arrays
  double* t = nullptr;           // the forward sums
  double structBytes = 0.0;      // the sweep structure as one apply reads it
  double halfBytes[2] = { 0.0, 0.0 }; // each half over all its chunks (a sweep from a guess reads both: sgs_apply_guess)
  uint32_t rowsBackward = 0;     // rows of the colours 0 .. nC - 2
};

namespace {
// CSR over device rows, a row's entries in the order they are summed: the matrix in device numbering entry for entry as stored
// (sgs_download; padding included), or a transfer operator's kept entries (sbhip_mg_fw.inc.h)
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
// old row -> device row of a matrix (identity unless Sell-C-sigma permuted)
std::vector<uint32_t> old_to_device_rows(const sb_matrix* m)
{
  std::vector<uint32_t> o2n(m->nr);
  if (m->fmt == 1 && m->permuted) {
    if (m->nr) sb_d2h(o2n.data(), m->oldToNew, (size_t)m->nr * sizeof(uint32_t));
  } else {
    for (uint32_t i = 0; i < m->nr; i++) o2n[i] = i;
  }
  return o2n;
}

// The one packer of the preconditioners' Sell-64 gather structures (SellRows, sgs.hip.h).  slotRow: per slot (a multiple of 64
// of them) the row of R it holds, 0xFFFFFFFF for none; keep(i, q): whether entry q of row i goes in.  Per slot the kept
// entries' count, per chunk their maximum, chunkPtr its prefix sum (handed back: the byte models read it), col / val
// column-major per chunk in R's order; padding is (+0.0, column 0) and is never used (the lane's own length stops it)
template <class Keep>
SellRows sell64_pack(const HostRows& R, const std::vector<uint32_t>& slotRow, Keep keep, std::vector<unsigned long long>& chunkPtr)
{
  const size_t slots = slotRow.size(), nChunks = slots / 64u;
  std::vector<uint32_t> rowLen(slots, 0), chunkLen(nChunks, 0);
  for (size_t sl = 0; sl < slots; sl++) {
    const uint32_t i = slotRow[sl];
    if (i == 0xFFFFFFFFu) continue;
    uint32_t len = 0;
    for (size_t q = R.ptr[i]; q < R.ptr[i + 1]; q++) len += keep(i, q) ? 1u : 0u;
    rowLen[sl]         = len;
    chunkLen[sl / 64u] = std::max(chunkLen[sl / 64u], len);
  }
  chunkPtr.assign(nChunks + 1, 0);
  for (size_t c = 0; c < nChunks; c++) chunkPtr[c + 1] = chunkPtr[c] + (unsigned long long)chunkLen[c] * 64u;
  std::vector<uint32_t> col(chunkPtr[nChunks], 0);
  std::vector<double> val(chunkPtr[nChunks], 0.0);
  for (size_t sl = 0; sl < slots; sl++) {
    const uint32_t i = slotRow[sl];
    if (i == 0xFFFFFFFFu) continue;
    size_t o = chunkPtr[sl / 64u] + (sl & 63u);
    for (size_t q = R.ptr[i]; q < R.ptr[i + 1]; q++)
      if (keep(i, q)) col[o] = R.col[q], val[o] = R.val[q], o += 64;
  }
  SellRows S;
  S.chunkPtr = sgs_to_device(chunkPtr), S.chunkLen = sgs_to_device(chunkLen), S.rowLen = sgs_to_device(rowLen);
  S.col = sgs_to_device(col), S.val = sgs_to_device(val);
  return S;
}
void sell64_free(SellRows& S)
{
  sb_free((void*)S.chunkPtr), sb_free((void*)S.chunkLen), sb_free((void*)S.rowLen), sb_free((void*)S.col), sb_free((void*)S.val);
  S = {};
}
// bytes a kernel reads of `chunks` chunks that hold `elements` elements: val + col per element; chunkPtr, chunkLen per chunk;
// per slot rowLen alone (4: slot == row) or rowLen and a row index beside it (8)
double sell64_bytes(unsigned long long elements, size_t chunks, int slotBytes)
{
  return (double)elements * 12.0 + (double)chunks * (64.0 * slotBytes + 12.0);
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
  // in storage order
  for (int up = 0; up < 2; up++) {
    auto in_half = [&](uint32_t i, size_t q) {
      const uint32_t ci = P->colour[i], cj = P->colour[h.col[q]];
      if (ci == cj) SB_FATAL("%s: device rows %u and %u are adjacent and share colour %u", who, i, h.col[q], ci);
      return up ? cj > ci : cj < ci;
    };
    std::vector<unsigned long long> chunkPtr;
    P->half[up] = sell64_pack(h, rowIdx, in_half, chunkPtr);
    // what one apply reads of it: the backward sweep leaves the last colour's chunks alone
    const uint32_t chunksRead = up ? (nC ? P->chunk0[nC - 1] : 0) : P->nChunks;
    P->structBytes += sell64_bytes(chunkPtr[chunksRead], chunksRead, 8);
    P->halfBytes[up] = sell64_bytes(chunkPtr[P->nChunks], P->nChunks, 8);
  }
  P->t = (double*)sb_malloc((size_t)nr * sizeof(double) + 4096);
  return P;
}

static void sgs_free_plan(SgsPlan* P)
{
  if (!P) return;
  sb_free(P->rowIdx), sb_free(P->t);
  for (SellRows& H : P->half) sell64_free(H);
  delete P;
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
}

// the forward sweep from the guess in z (both halves of the plan, t kept), then the backward sweep as the apply's
static void sgs_apply_guess(const SgsPlan* P, const double* dinv, const double* r, double* t, double* z, const int* stop)
{
  for (uint32_t c = 0; c < P->nC; c++)
    hipLaunchKernelGGL(mg_sweep_guess_k, sgs_grid(P, c), dim3(256), 0, g.stream, P->chunk0[c], P->chunk0[c + 1] - P->chunk0[c],
        (const uint32_t*)P->rowIdx, P->half[0], P->half[1], r, dinv, t, z, stop);
  sgs_backward(P, dinv, t, z, stop);
}

// bytes one apply reads and writes: the sweep structure, and per row forward r, dinv, one gathered z in, t, z out; backward (the
// rows of every colour but the last) t, dinv, one gathered z in, z out
static double sgs_bytes(const SgsPlan* P, uint32_t nr) { return P->structBytes + 40.0 * (double)nr + 32.0 * (double)P->rowsBackward; }
