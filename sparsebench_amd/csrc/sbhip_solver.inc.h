// sbhip_solver.inc.h -- part of the single translation unit sbhip.hip (textual include, shares its static context): the host
// plumbing every solver handle repeats around its own kernels ("One definition per solver plumbing step").  Plain
// functions; what a solver does between them (its prologue, body and epilogue) stays in its own file.
// ===========================================================================
// solver plumbing
// ===========================================================================

// --- refusals at create / start -------------------------------------------------------------------------------------------
static void need_dp(const sb_matrix* m, const char* fn, const char* who)
{
  if (m->prec != 2) SB_FATAL("%s: %s: double precision only (the matrix was uploaded in single precision)", fn, who);
}
// halo: NULL where the entry point ignores its halo plan
static void need_one_rank(const sb_matrix* m, const sb_halo* halo, const char* fn, const char* who)
{
  if (multi_rank() || sb_comm_size() > 1 || m->nc != m->nr || (halo && halo->externalCount > 0))
    SB_FATAL("%s: %s runs on one rank (this process is rank %d of %d, the matrix has %u halo columns)", fn, who, g.rank, g.size,
        m->nc - m->nr);
}
// seq_owner: whose validation mode the sequential order is, as the message names it
static void need_tree(const char* fn, const char* who, const char* seq_owner)
{
  if (sb_dot_order() == 1)
    SB_FATAL("%s: %s runs in the tree dot order only (the process is in the seq order: SB_DOT_ORDER=seq / sb_set_dot_order(1), "
             "the validation mode of %s)", fn, who, seq_owner);
}
// what: "vectors" or "block vectors"
static void need_aligned16(std::initializer_list<const void*> ptrs, const char* fn, const char* what)
{
  uintptr_t bits = 0;
  for (const void* q : ptrs) bits |= (uintptr_t)q;
  if (bits & 15u) SB_FATAL("%s: %s must be 16-byte aligned", fn, what);
}

// --- vectors between the caller's row order and the device's ----------------------------------------------------------------
static void upload_permuted(const sb_matrix* m, const double* host, double* dev)
{
  if (m->nr == 0) return;
  double* tmp = scratch_ws(0, m->nr);
  sb_h2d(tmp, host, (size_t)m->nr * sizeof(double));
  sb_permute(m, tmp, dev);
  HIP_CHECK(hipStreamSynchronize(g.stream));
}
static void download_original(const sb_matrix* m, const double* dev, double* host)
{
  if (m->nr == 0) return;
  double* tmp = scratch_ws(1, m->nr);
  sb_unpermute(m, dev, tmp);
  sb_d2h(host, tmp, (size_t)m->nr * sizeof(double));
}

// --- device control blocks ------------------------------------------------------------------------------------------------
template <class S> static S zeroed()
{
  S h;
  memset(&h, 0, sizeof h);
  return h;
}
// both wait for the stream first: the block is read and written by the kernels in flight
template <class S> static S read_block(const S* dev)
{
  HIP_CHECK(hipStreamSynchronize(g.stream));
  S h;
  HIP_CHECK(hipMemcpy(&h, dev, sizeof h, hipMemcpyDeviceToHost));
  return h;
}
template <class S> static void write_block(S* dev, const S* h, size_t count = 1)
{
  HIP_CHECK(hipStreamSynchronize(g.stream));
  HIP_CHECK(hipMemcpy(dev, h, sizeof(S) * count, hipMemcpyHostToDevice));
}
// a throw-away control block for a blocking test entry: test_block | the kernel launch | test_block_done
template <class S> static S* test_block(const S& h)
{
  S* dev = (S*)sb_malloc(sizeof h);
  write_block(dev, &h);
  return dev;
}
template <class S> static void test_block_done(S* dev)
{
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(g.stream));
  sb_free(dev);
}

// --- the loop between *_start and *_finish ----------------------------------------------------------------------------------
// start ends with begin(); finish records end(), enqueues and waits for its epilogue, then read()s
namespace {
struct LoopClock {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  float ms      = 0.f;
  bool open     = false; // between begin() and read()
  void create()
  {
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
  }
  void destroy()
  {
    HIP_CHECK(hipEventDestroy(e0));
    HIP_CHECK(hipEventDestroy(e1));
  }
  void begin()
  {
    ms = 0.f, open = true;
    HIP_CHECK(hipEventRecord(e0, g.stream));
  }
  void end() { HIP_CHECK(hipEventRecord(e1, g.stream)); }
  void read() // after the stream has been waited for
  {
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    open = false;
  }
  void need_open(const char* fn, const char* start_fn) const
  {
    if (!open) SB_FATAL("%s before %s", fn, start_fn);
  }
};
} // namespace

// bodies of a whole solve: the reference's loop runs k = 1 .. itermax - 1 (src/CGSolver.c:107)
static int loop_bodies(int itermax) { return itermax > 1 ? itermax - 1 : 0; }

// --- histories --------------------------------------------------------------------------------------------------------------
// room for `per` histories of `want` entries each where `have` entries are not enough (the contents are not kept)
static void grow(double*& buf, int have, int want, size_t per)
{
  if (want <= have) return;
  sb_free(buf);
  buf = (double*)sb_malloc(per * (size_t)want * sizeof(double));
}
// the first min(have, hist_cap, cap) entries; returns the entries copied
static int copy_history(const double* dev, int have, int hist_cap, double* out, int cap)
{
  const int cnt = std::min(std::min(have, hist_cap), cap);
  if (cnt <= 0) return 0;
  HIP_CHECK(hipMemcpy(out, dev, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost));
  return cnt;
}

// --- max|x - xexact| on this rank (solverCheckResidual, src/CGSolver.c:40-60); 0.0 without an exact solution ----------------
static double max_abs_diff_host(uint32_t n, const double* x, const double* xexact)
{
  if (!xexact || n == 0) return 0.0;
  const uint32_t blocks = stream_grid(n, 256);
  double* q             = scratch_partials(blocks);
  hipLaunchKernelGGL(max_abs_diff_partials, dim3(blocks), dim3(256), 0, g.stream, n, x, xexact, q);
  HIP_CHECK(hipGetLastError());
  std::vector<double> h(blocks);
  sb_d2h(h.data(), q, blocks * sizeof(double));
  double mx = 0.0;
  for (double v : h)
    if (v > mx) mx = v;
  return mx;
}

// --- M^-1 for a solver that borrows a PCG handle's preconditioner --------------------------------------------
// BiCGStab and GMRES each hold one.  M^-1 is a diagonal (dinv, the holder's own allocation: a copy of a plan-less PCG handle's,
// or the caller's) or precond_cycle on the plan of the borrowed handle M: V(0, .), bit for bit sb_pcg_apply_precond's.  A plan's
// level vectors are the cycle's scratch, so every handle on M and M's own solves take turns.  The members are defined beside
// precond_cycle (sbhip_mg.inc.h).
struct sb_pcg;
struct PrecondPlan;
namespace {
// what the kernel that PRODUCES a vector writes of M^-1 of it on the way out (pre_first<mode>, kernels.hip.h): -1 nothing (the
// sweeps; no preconditioner), 0 a diagonal's product with dinv, 1 the polynomial's step 1 into level 0's d and the destination
struct PrecondRide {
  int mode           = -1;
  const double* dinv = nullptr;
  double* d          = nullptr;
  double c1          = 0.0;
};
struct RightPrecond {
  const sb_pcg* M         = nullptr; // borrowed with its plan; NULL for a diagonal
  const PrecondPlan* plan = nullptr;
  double* dinv            = nullptr; // a diagonal's entries, device row order (the holder frees them)
  // the refusals of a *_create_pre entry point fn (no handle, another matrix, a solve open); nothing is taken yet
  static void need_borrowable(const sb_matrix* m, const sb_pcg* M, const char* fn);
  // M's plan, or (a plan-less M) a copy of its dinv in `bytes` of the holder's own, after which M is not referred to again
  void borrow(const sb_pcg* M, size_t bytes);
  void need_closed(const char* fn) const; // at every *_start: not while M's own solve has the plan's vectors in flight
  bool set() const { return plan || dinv; }
  int kind() const;                 // 0: a diagonal; else the plan's kind as sb_pcg_precond reports it
  const double* diagonal() const;   // dinv, or level 0's of the plan
  PrecondRide ride() const;
  // dst = M^-1 src over n rows.  rode: src's producer has written ride()'s part; else everything is made here
  void apply(uint32_t n, const double* src, double* dst, const int* stop, bool rode) const;
  int apply_launches() const; // of an apply behind a producer that rode
};
} // namespace

// --- grid of the 1024-thread streaming kernels over n rows (cg_update_r_k<0>'s, dot_l1_k's): a wave per 256-row group, two
// workgroups per CU at most ------------------------------------------------------------------------------------------------
static uint32_t vec_stream_grid(uint32_t n)
{
  const uint32_t nGroups = (n + 255u) >> 8;
  return std::max(1u, std::min((uint32_t)g.prop.multiProcessorCount * 2u, (nGroups + 15u) / 16u));
}
