/* sbhip.h -- the C-ABI of the MI355X (gfx950) HIP layer for SparseBench's CG hot path.
 *
 * Plain C: opaque handles, pointers and sizes only.  This is what a host program
 * written in the reference's language (C) binds; the reference-shaped symbols
 * (convertMatrix, spMVM, waxpby, ddot, solveCG, commExchange, commReduction --
 * see include/sparsebench/) are thin C wrappers over these entry points, and
 * INTEGRATION.md shows the binding a SparseBench maintainer would add.
 *
 * Conventions (mirroring the reference):
 *  - one process drives one GPU; all calls come from that process's main thread
 *    (reference: src/profiler.c:17 globals, single-threaded API use);
 *  - errors are fatal: message with file:line on stderr, then exit(EXIT_FAILURE)
 *    (reference: src/allocate.c:19-33, src/matrix.c:129-170) -- no error codes;
 *  - CG_FLOAT = double, CG_UINT = unsigned int (reference defaults,
 *    src/util.h:35-53, config.mk:7-8);
 *  - every vector pointer is a DEVICE pointer unless the name says host;
 *  - work is enqueued on the layer's own HIP stream; calls that return a value to
 *    the host synchronise that stream, the others do not.
 *
 * Each entry point cites the reference interface it replaces (paths relative to
 * the reference root).
 */
#ifndef SBHIP_H
#define SBHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sb_matrix sb_matrix; /* device-resident sparse matrix (CRS or SCS) */
typedef struct sb_halo sb_halo;     /* device-resident halo plan of this rank     */
typedef struct sb_cg sb_cg;         /* CG solver state (vectors + scalars in HBM) */
typedef struct sb_gmres sb_gmres;   /* restarted GMRES(m) state (Krylov basis + scalars in HBM) */

/* ---- context ------------------------------------------------------------- */
/* replaces: commInit's process setup, src/comm.c:863-878 (device instead of rank) */
void sb_init(int device);
void sb_finalize(void);
int sb_is_initialized(void);
int sb_device_count(void);
const char* sb_device_name(void); /* e.g. "AMD Instinct MI355X (gfx950)" */
int sb_num_cus(void);
void sb_sync(void);      /* wait for the layer's stream */
void* sb_stream(void);   /* the hipStream_t, for callers that want to order work */

/* replaces: allocate(), src/allocate.h:9 -- for arrays that live on the hot path */
void* sb_malloc(size_t bytes);
void sb_free(void* dev);
void sb_memset(void* dev, int byte, size_t bytes);
void sb_h2d(void* dev, const void* host, size_t bytes); /* synchronous */
void sb_d2h(void* host, const void* dev, size_t bytes); /* synchronous */
void sb_d2d(void* dst, const void* src, size_t bytes);  /* stream-ordered */
int sb_is_device_ptr(const void* p);
/* replaces: allocate() AS THE DRIVER USES IT, src/allocate.c:12-36 + src/main.c:205-211 -- vectors the caller fills with host
 * loops and then hands to spMVM.  Memory in HBM that the CPU can store to (fine-grained device memory through the PCIe BAR) and
 * kernels read in place; NULL where the one-time probe says this box cannot do that (sb_host_visible_reason() tells why either
 * way; SPARSEBENCH_ALLOCATE=host switches it off).  sb_is_device_ptr() is 1 for it; free with sb_free(). */
void* sb_malloc_host_visible(size_t bytes);
const char* sb_host_visible_reason(void);
void* sb_malloc_pinned_host(size_t bytes); /* fallback: pinned host memory (staged by spMVM / waxpby / ddot); NULL on failure */
void sb_free_pinned_host(void* p);
int sb_is_pinned_host_ptr(const void* p); /* 1: memory from hipHostMalloc (sb_malloc_pinned_host) */
size_t sb_mem_free_bytes(void);           /* free device memory (hipMemGetInfo) */
/* host <-> device copies made through sb_h2d / sb_d2h so far: {h2d calls, h2d bytes, d2h calls, d2h bytes} */
void sb_copy_counters(uint64_t out[4]);

/* stream-ordered timing (PROFILE macro, src/profiler.h:18-21, needs completion) */
void* sb_event_create(void);
void sb_event_record(void* ev);
float sb_event_elapsed_ms(void* start, void* stop); /* synchronises on stop */
void sb_event_destroy(void* ev);
/* replaces: the PROFILE macro's host clock, src/profiler.h:18-21 -- a region (tag 0..7) bracketed by two events on the layer's
 * stream, nothing waits inside the caller's loop; sb_region_seconds() waits for what is outstanding and returns the accumulated
 * DEVICE time of the tag and how many regions were recorded. */
void sb_region_begin(int tag);
void sb_region_end(int tag);
double sb_region_seconds(int tag, uint64_t* count);
void sb_region_reset(void);

/* ---- matrix upload (device side of convertMatrix, src/matrix.h:57) -------- */
/* CRS: src/CRSMatrix.h:9-16.  Arrays are host pointers, copied to HBM. */
sb_matrix* sb_crs_upload(uint32_t nr, uint32_t nc, const uint32_t* rowPtr,
                         const uint32_t* colInd, const double* val);
/* Sell-C-sigma: src/SCSMatrix.h:13-27, host layout exactly as the reference's
 * convertMatrix builds it (src/matrix-SCS.c:31-196; columns NOT permuted).
 * For sigma > 1 the device copy of colInd is renumbered to the permuted row order
 * (symmetric permutation) so the CG vectors can live in permuted order. */
sb_matrix* sb_scs_upload(uint32_t nr, uint32_t nc, uint32_t C, uint32_t sigma,
                         uint32_t nChunks, uint32_t nElems, const uint32_t* chunkPtr,
                         const uint32_t* chunkLens, const uint32_t* colInd, const double* val,
                         const uint32_t* oldToNewPerm, const uint32_t* newToOldPerm);
void sb_matrix_free(sb_matrix* m);
/* Where the reference-layout stream (val, colInd: what spMVM of src/matrix-SCS.c:198-228 / src/matrix-CRS.c:46-65 reads) sits
 * in device memory: one slab, the two arrays at the given offsets (0..256 MB each) inside their regions of it.  The same kernel
 * streams the same bytes 10-20 % faster or slower depending on WHICH memory that is; sb_scs_upload / sb_crs_upload
 * pick it by measurement, together with the memory of the CG loop's vectors (SB_PLACE=0: everything stays where hipMalloc put
 * it).  The calls below (down to sb_placement_probe) are lab calls for uploads made with SB_PLACE=0 (tools/placement_lab*.py). */
void sb_matrix_place(sb_matrix* m, int colOffMB, int valOffMB);
void sb_matrix_place_fresh(sb_matrix* m); /* the same arrays in a NEW slab; earlier slabs stay allocated until the commit */
void sb_matrix_place_commit(sb_matrix* m);
void sb_matrix_placement(const sb_matrix* m, int out[2]); /* {-1, -1}: not placed */
void sb_matrix_place_at(sb_matrix* m, void* colMem, void* valMem); /* lab: the stream copied to the caller's memory */
void sb_matrix_place_home(sb_matrix* m);                            /* lab: back to the first upload */
size_t sb_placement_arena_bytes(const sb_matrix* m);                /* lab: bytes of the loop's vector layout */
float sb_placement_probe(sb_matrix* m, void* arena);                /* lab: the tuner's proxy step (us) with the vectors at `arena` */
int sb_matrix_placement_report(const sb_matrix* m, float us[3]); /* probes the upload's tuner timed; us of a proxy loop body: first arena + hipMalloc's placement, the pair kept, the slowest */
void sb_matrix_debug_ptrs(const sb_matrix* m, unsigned long long out[4]); /* lab: device addresses of colInd, val, chunkPtr | rowPtr, chunkLens */
uint32_t sb_matrix_nr(const sb_matrix* m);
uint32_t sb_matrix_nc(const sb_matrix* m);
int sb_matrix_is_permuted(const sb_matrix* m); /* 1 for SCS with a non-identity row sort */
/* algorithmic bytes one SpMV moves:
 *   CRS 12*nnz + 4*(nr+1) + 8*nr + 8*nc ; SCS 12*nElems + 8*nChunks + 8*nrPadded + 8*nc */
double sb_matrix_spmv_bytes(const sb_matrix* m);
/* SCS C=64 matrices also get a device-private LOSSLESS compressed mirror at upload
 * (csrc/pack.hip.h; SB_PACK=0 disables it): level 1 = 16-bit column offsets per chunk,
 * level 2 = additionally a <=256-entry value dictionary.  Results are bit-identical to
 * the uncompressed kernel; the host-visible arrays keep the reference layout. */
/* Optional, before an upload of a rank-local matrix: the global ids of its halo columns (local column nr + i has
 * global id global_ids[i]; commPartition's Comm::externalGlobal).  Used only to lay out device-private x windows
 * (the partitioner numbers halo columns in the order it met them; in ascending global order a stencil's halo
 * plane looks like the rank's own planes and the pattern levels apply to the tiles next to a rank boundary).
 * Stays in force until replaced (n = 0 clears); uploads whose nc - nr differs from n ignore it. */
void sb_set_external_ids(const uint32_t* global_ids, uint32_t n);
int sb_matrix_pack_level(const sb_matrix* m);
/* select the SpMV kernel at run time.  There are two: 0 the reference-layout stream, 5 the masked row programs (level 6:
 * every chunk of a tile stored as a masked row program; built when >= 98 % of the chunks' rows are sub-sequences of a row
 * of their tile; SB_PACK < 6 builds none) where the matrix has them (the default then).  Any request below 5, or 5 on a
 * matrix without row programs, selects 0.  Levels 1-5 are still built on the way to level 6 (sb_matrix_pack_level and the
 * counts below report them); their own kernels were measured slower and removed.  Both kernels give
 * bit-identical results. */
/* CRS matrices: 0 = native CRS kernel, 5 = product through a device-private Sell-64-1 pattern mirror whose
 * padding is not added (exactly the CRS loop's sums); built when the matrix has repeating row patterns. */
void sb_matrix_use_packed(sb_matrix* m, int mode);
int sb_matrix_packed_mode(const sb_matrix* m);
/* which native CRS kernel streams the reference's arrays (pack mode 0): 1 spmv_crs_split -- equal windows of nonzeros, the
 * default where no row is longer than 1025 --, 0 spmv_crs_stream (row blocks; SB_CRS_KERNEL=stream forces it).  Both:
 * src/matrix-CRS.c:46-65, same bits. */
int sb_matrix_crs_kernel(const sb_matrix* m);
uint32_t sb_matrix_lds_window(const sb_matrix* m); /* doubles per workgroup, 0 if not built */
uint32_t sb_matrix_pattern_classes(const sb_matrix* m); /* pattern tables built (mode 3), 0 if none */
/* mode 3, level 5: distinct shared row patterns; *uniformChunks = chunks stored as one row
 * pattern + exception lanes (the rest keep per-lane codes).  SB_PACK=4 builds none. */
uint32_t sb_matrix_row_patterns(const sb_matrix* m, uint32_t* uniformChunks);
/* mode 5, level 6: distinct masked row programs; *maskedChunks = chunks stored as one program + per-row base slots
 * (every lane runs the program, each add under the mask of the lanes that have the entry).  0 if not built
 * (SB_PACK=5 builds none; fewer than 98 % of the chunks qualifying: not kept). */
uint32_t sb_matrix_row_programs(const sb_matrix* m, uint32_t* maskedChunks);
/* bytes the selected SpMV kernel really moves per launch (stream + x + y) */
double sb_matrix_stream_bytes(const sb_matrix* m);
/* Sell-64, double precision, reference-layout kernel (mode 0): k sixteenths of the stream's 4-chunk blocks, evenly
 * interleaved, are read with plain loads and so stay in the 256 MiB Infinity Cache from one SpMV to the next; the rest is read
 * non-temporally.  The upload sets k from the stream's bytes, the loop's vector bytes (4 vectors of nc doubles) and the
 * cache size; it is 0 where ranks share a device and where the vectors alone exceed the cache.  k = -1 selects that rule
 * again, 0 ... 16 forces a share (tests, A/B measurements); the share in force is returned (0 for any other matrix).  Every
 * share gives the same bits. */
int sb_matrix_resident_share(sb_matrix* m, int k);
/* the rule itself (host arithmetic only): the share for a stream of streamBytes and vectors of nc doubles */
int sb_resident_share_rule(double streamBytes, uint32_t nc, int sharedDevice);
/* either precision: 1 when the matrix (CRS: its private mirror) has row programs for EVERY chunk, no class dictionary and
 * only mapped or simple windows -- what the SpMV with the p update inside needs of a matrix, and the condition under which a
 * single-precision upload keeps its mirror (sb_set_sp_mirror): for an SP matrix 1 exactly when the mirror was built and kept. */
int sb_matrix_all_row_programs(const sb_matrix* m);

/* ---- kernels ---------------------------------------------------------------- */
/* spMVM, src/solver.h:13: y = A x, x has nc entries, y has nr entries, both in
 * the caller's (original) row order for every format and sigma. */
void sb_spmv(const sb_matrix* m, const double* x, double* y);
/* the SCS fast path used inside CG: x and y in the matrix's permuted row order
 * (identical to sb_spmv when sb_matrix_is_permuted() == 0) */
void sb_spmv_native(const sb_matrix* m, const double* x, double* y);
/* sb_spmv_native plus, fused into the same launch, the partial sums of the dot product x . y in the canonical order of
 * DESIGN 4.3 (rows of the device's order) -- what the CG loop does for p . Ap.  Returns which values partials_dev holds:
 *   0  nothing: the selected kernel has no fused dot (Sell-C-sigma with C != 64, native CRS);
 *   2  LEVEL-1 values, one per aligned 256 rows = ((q0 + q1) + q2) + q3 of four level-0 partials: ceil(nr / 256) doubles
 *      (reference-layout Sell-64 stream and masked row programs -- a block / tile combines its chunks itself, so the
 *      scalar step that follows reads a quarter of the bytes through its single CU).
 * partials_dev: 4 * ceil(nr / 256) doubles, zero-filled by the caller (entries behind the last group stay +0.0). */
int sb_spmv_native_dot(const sb_matrix* m, const double* x, double* y, double* partials_dev);
/* vector <-> permuted order of an SCS matrix: out[new] = in[old] / out[old] = in[new] */
void sb_permute(const sb_matrix* m, const double* in_orig, double* out_perm);
void sb_unpermute(const sb_matrix* m, const double* in_perm, double* out_orig);

/* waxpby, src/solver.h:15-20: w = alpha*x + beta*y (w may alias x or y) */
void sb_waxpby(uint32_t n, double alpha, const double* x, double beta, const double* y,
               double* w);
/* ddot, src/solver.h:22-25 (+ commReduction SUM when a communicator is attached).
 * Fixed summation order (DESIGN.md "dot order"): bit-reproducible run to run. */
void sb_ddot_async(uint32_t n, const double* x, const double* y, double* result_dev);
double sb_ddot(uint32_t n, const double* x, const double* y); /* synchronises */
/* the stages of the fixed order, exposed for parity tests: level 0 writes one partial per
 * 64 elements into partials_dev[0 .. 4*ceil(n/256)) (tail zeroed); sb_reduce_final does
 * levels 1-2 over m = ceil(n/256) groups of four partials */
void sb_ddot_partials(uint32_t n, const double* x, const double* y, double* partials_dev);
void sb_reduce_final(uint32_t m, const double* partials_dev, double* result_dev);
/* The dot order of sb_ddot, sb_ddot_async and of every solver that does not choose its own (sb_cg_set_dot_order):
 * 0 = tree, the fixed order above (the default); 1 = seq, the reference's own ddot (src/solver.c:41-62 as shipped,
 * ENABLE_OPENMP = false): per rank ONE left-to-right sum `sum = 0.0; sum += x[i] * y[i]` over its rows in original row
 * order, every product rounded before its add, the ranks' sums then combined as in tree order.  seq runs on one
 * workgroup (a dependent add per element) and exists for validation: with it the GPU reproduces the reference's
 * numbers bit for bit.  SB_DOT_ORDER=tree|seq sets the default at the first call (any other value ends the process with
 * a message); sb_dot_order works before sb_init.  sb_ddot_partials / sb_reduce_final stay the tree order's stages. */
void sb_set_dot_order(int order);
int sb_dot_order(void);

/* ---- single precision: the reference's FLOAT_TYPE=SP build (src/util.h:47-51, -DPRECISION=1) ---------------- */
/* CG_FLOAT = float everywhere: values, vectors and every operation; each product rounded to float before its add, sums
 * accumulate in float, f32 subnormals kept.  By default an SP matrix streams the reference layout only (no placement tuner
 * either); sb_set_sp_mirror below opts into the compressed mirror with masked row programs in float.  Any number of ranks: sb_halo_exchange_f32 / sb_comm_reduction_f32 and the CG loop's
 * float halo and float all-reduce on both data planes.  Crossing precisions -- an fp64 entry point on an
 * SP matrix or solver, or the other way round -- is a fatal error with file:line. */
/* The SP mirror switch (opt-in, off by default): while it is on, sb_crs_upload_f32 / sb_scs_upload_f32 also build the
 * device-private mirror of the fp64 path (Sell-C-sigma with C = 64; CRS through its private Sell-64-1 mirror) with the
 * program values and the x window in float, and keep it if EVERY chunk became a row program (sb_matrix_all_row_programs);
 * otherwise the matrix is exactly what an upload with the switch off makes.  A matrix keeps what it was built with.  With a
 * mirror the default kernel mode is 5 at every size, sb_matrix_use_packed(m, 0 / 5) selects, sb_spmv_native_dot_f32 returns
 * level-1 values for CRS too, and the one-rank fused CG loop takes the p update inside the SpMV (3 launches per body;
 * sb_cg_set_fuse_p / SB_FUSE_P=0 turn that off).  Same bits as the streaming kernels everywhere.
 * SB_SP_MIRROR=0|1 sets the process default at the first call (any other value, or an argument other than 0 / 1, ends the
 * process with a message); sb_sp_mirror works before sb_init.  SB_SP_MIRROR_REPORT=1: every SP upload prints one line to
 * stderr: SP_MIRROR built=<0|1> fmt=<crs|scs> chunks=<n> programs=<n> window=<slots> reason=<text>. */
void sb_set_sp_mirror(int on);
int sb_sp_mirror(void);
sb_matrix* sb_crs_upload_f32(uint32_t nr, uint32_t nc, const uint32_t* rowPtr, const uint32_t* colInd, const float* val);
sb_matrix* sb_scs_upload_f32(uint32_t nr, uint32_t nc, uint32_t C, uint32_t sigma, uint32_t nChunks, uint32_t nElems,
                             const uint32_t* chunkPtr, const uint32_t* chunkLens, const uint32_t* colInd, const float* val,
                             const uint32_t* oldToNewPerm, const uint32_t* newToOldPerm);
int sb_matrix_precision(const sb_matrix* m); /* 1 single, 2 double (the reference's PRECISION values) */
void sb_spmv_f32(const sb_matrix* m, const float* x, float* y); /* as sb_spmv */
/* as sb_spmv_native_dot: 2 = the LEVEL-1 values of x . y (Sell-64, and CRS through a selected mirror; ceil(nr / 256) floats),
 * 0 = none (y only) */
int sb_spmv_native_dot_f32(const sb_matrix* m, const float* x, float* y, float* l1_dev);
void sb_permute_f32(const sb_matrix* m, const float* in_orig, float* out_perm);
void sb_unpermute_f32(const sb_matrix* m, const float* in_perm, float* out_orig);
void sb_waxpby_f32(uint32_t n, float alpha, const float* x, float beta, const float* y, float* w); /* src/solver.c:16-39 */
/* ddot in float, in the process dot order (sb_dot_order): tree = the levels of sb_ddot_partials / sb_reduce_final, in float;
 * seq = `CG_FLOAT sum = 0.0; sum += x[i] * y[i]` left to right.  Synchronises. */
float sb_ddot_f32(uint32_t n, const float* x, const float* y);
void sb_ddot_partials_f32(uint32_t n, const float* x, const float* y, float* partials_dev); /* level 0: 4*ceil(n/256) floats */
void sb_reduce_final_f32(uint32_t m, const float* partials_dev, float* result_dev);          /* levels 1-2 over m groups */
/* solveCG in single precision (src/CGSolver.c:62-141 of the SP build): b_host / xexact_host are nr floats.  Every other
 * sb_cg_* call serves both precisions; sb_cg_history returns the float values exactly in its double arrays. */
sb_cg* sb_cg_create_f32(const sb_matrix* m, sb_halo* halo, const float* b_host, const float* xexact_host);
void sb_cg_solution_f32(const sb_cg* s, float* x_host);

/* ---- multi-GPU (one rank per GPU, RCCL over xGMI) ---------------------------- */
/* replaces MPI_Init / MPI_COMM_WORLD.  id = 128-byte ncclUniqueId made by rank 0
 * with sb_comm_unique_id() and handed to the other ranks by the launcher. */
#define SB_UNIQUE_ID_BYTES 128
void sb_comm_unique_id(void* id_out);
void sb_comm_init(int rank, int size, const void* id);
/* Alternative to RCCL: a host-mediated transport supplied by the launcher (MPI without
 * GPU awareness, gloo, ...).  Also what lets the N-rank device path be exercised by several
 * processes sharing ONE GPU (tests/test_gpu_multirank.py).  Callbacks are entered with the
 * layer's stream synchronised, get DEVICE pointers, and return when those are written. */
typedef struct {
  void* ctx;
  /* commReduction: in place on one double; op 0 = MAX, 1 = SUM */
  void (*allreduce)(void* ctx, double* v_dev, int op);
  /* commExchange after packing: send_dev[sdispls[i] .. +sendCounts[i]) goes to destinations[i];
   * recv_dev[rdispls[j] .. +recvCounts[j]) comes from sources[j] */
  void (*neighbour_exchange)(void* ctx, const double* send_dev, int outdegree, const int* destinations,
                             const int* sendCounts, const int* sdispls, double* recv_dev, int indegree,
                             const int* sources, const int* recvCounts, const int* rdispls);
  /* optional (may be NULL): all_host[r * nbytes ..] = rank r's mine_host; lets the layer set up the
   * exchange over peer-mapped memory (halo staging areas) on top of this transport.  Single precision on
   * several ranks needs it: the float all-reduce gathers the ranks' floats through it (sb_comm_reduction_f32);
   * without it the SP uploads and sb_cg_create_f32 end the process with a message */
  void (*allgather_bytes)(void* ctx, const void* mine_host, int nbytes, void* all_host);
} sb_transport;
void sb_comm_init_transport(int rank, int size, const sb_transport* t);
/* In-kernel all-reduce of the CG scalars over peer-mapped memory (one launch per dot instead of
 * local reduce | ncclAllReduce | scalar step).  Every rank owns a small fine-grained buffer that
 * its peers map through HIP IPC.  sb_comm_init does this by itself (the handles travel over RCCL).
 * A launcher with its own transport calls sb_comm_p2p_handle on every rank, gathers the
 * SB_P2P_HANDLE_BYTES of all ranks in rank order, and calls sb_comm_p2p_open (collective): peers are
 * mapped, one exchange is tested, and the ranks agree over the transport; any failure on any rank
 * leaves every rank on the transport's all-reduce.  SB_P2P=0 disables.  Returns 1 when enabled. */
#define SB_P2P_HANDLE_BYTES 64
int sb_comm_p2p_handle(unsigned char* handle_out);
int sb_comm_p2p_open(const unsigned char* all_handles); /* NULL: this rank has no handle */
int sb_comm_p2p_enabled(void);
/* one line saying why the path is on or off (which rank, which call failed, what the self-test saw);
 * waits inside CG are bounded by SB_P2P_TIMEOUT_MS (default 30000), the set-up self-tests by 5 s */
const char* sb_comm_p2p_reason(void);
/* Which data plane the CG loop uses from now on: 1 (default) the peer-mapped paths where their set-up succeeded,
 * 0 the communicator's own collectives (all-reduce, send / recv: src/comm.c:640-648,659) although the mappings
 * exist -- as SB_P2P=0 SB_P2P_HALO=0 would have given, nothing torn down, so one process can time both (bench.py).
 * Collective by contract: every rank calls it with the same value, between solves; solver objects are created
 * after the switch. */
void sb_comm_data_plane(int peer_mapped);
int sb_comm_data_plane_selected(void);
/* Variant of the peer-mapped halo exchange: 1 = the halo push rides in the SpMV launch (its first workgroups send
 * p[elementsToSend], src/comm.c:635-638) instead of a launch of its own; 0 = separate push kernel (default;
 * SB_HALO_PUSH_INSIDE=1 changes the default).  Same bits.  Collective, between solves. */
void sb_comm_halo_push_inside(int on);
/* The peer-mapped halo exchange folded into the STREAMING loop's own kernels (Sell-C-sigma, C = 64, the reference-layout
 * kernel; double and single precision): 1 = the p update sends the boundary rows it has just written and the SpMV's blocks
 * that hold a halo column, dispatched last, wait for the neighbours' flags and read the staging area themselves -- no push
 * and no pull launch, 5 launches per body instead of 7; 0 = today's body (default; SB_HALO_FOLD=0|1 sets the process
 * default at the first use, any other value ends the process).  Same bits.  Its per-step time on ranks with a GPU each
 * is unmeasured.  sb_comm_halo_fold: collective, between solves, synchronises the layer's stream.
 * sb_comm_halo_fold_selected answers before sb_init.  A solve that cannot fold (one rank, the communicator's plane, CRS,
 * generic C, the row-program / mirror kernels, fused = 0, the seq dot order) silently keeps its body: sb_cg_halo_fold. */
void sb_comm_halo_fold(int on);
int sb_comm_halo_fold_selected(void);
/* what the RCCL communicator itself reports (ncclCommCount / ncclCommUserRank / ncclCommCuDevice):
 * out = {ranks, this rank, HIP device}; returns 0 (out = -1) without an RCCL communicator */
int sb_comm_rccl_info(int out[3]);
void sb_comm_finalize(void);
int sb_comm_rank(void);
int sb_comm_size(void);
/* commReduction, src/comm.h:58 (op: 0 = MAX, 1 = SUM as enum op, src/comm.h:25);
 * in place on one device double; stream-ordered */
void sb_comm_reduction(double* v_dev, int op);
/* commReduction of the SP build (MPI_FLOAT): in place on one device float.  Every plane adds the ranks' floats pairwise in
 * rank order, ((v0 + v1) + (v2 + v3)) + ..., in float -- MPICH's order -- so the bits do not depend on the plane or on P:
 * RCCL all-gathers the values (stream-ordered) and one thread adds them; a host transport all-gathers them with its
 * allgather_bytes (required) and the host adds them.  op 0 = MAX, 1 = SUM. */
void sb_comm_reduction_f32(float* v_dev, int op);
/* that rank reduction on the host: values[0 .. n) in rank order, op 0 = MAX, 1 = SUM (pairwise float tree) */
float sb_rank_reduce_f32(const float* values, int n, int op);
/* setup-time exchanges between ranks over the same communicator, host buffers in
 * and out (replace MPI_Allgather src/comm.c:496 and the Send/Irecv of wanted ids
 * src/comm.c:134-161) */
void sb_comm_allgather_bytes(const void* mine_host, int nbytes, void* all_host);
void sb_comm_alltoallv_ints(const int* sendbuf, const int* sendcounts, const int* sdispls,
                            int* recvbuf, const int* recvcounts, const int* rdispls);
void sb_comm_barrier(void);
/* device side of commPartition's result, src/comm.h:27-46: neighbour lists and
 * elementsToSend become device arrays.  perm_of_row may be NULL (identity). */
/* (test hook: SB_TEST_CORRUPT_HALO=r makes rank r send a wrong row's value in its first halo slot, announced on
 * stderr -- bench.py's pre-flight gate must catch it) */
sb_halo* sb_halo_create(uint32_t nr, int outdegree, const int* destinations,
                        const int* sendCounts, const int* sdispls, int indegree,
                        const int* sources, const int* recvCounts, const int* rdispls,
                        const int* elementsToSend, int totalSendCount, int externalCount,
                        const uint32_t* oldToNewPerm);
void sb_halo_free(sb_halo* h);
/* 1: inside CG this halo is exchanged by push / pull kernels over peer-mapped staging areas (set up
 * collectively in sb_halo_create when the in-kernel all-reduce is on; SB_P2P_HALO=0 disables), 0: RCCL /
 * transport send-recv */
int sb_halo_p2p_enabled(const sb_halo* h);
const char* sb_halo_p2p_reason(const sb_halo* h);
/* commExchange, src/comm.h:57: pack x[elementsToSend] and deliver every
 * neighbour's slice into x[numRows ...]; stream-ordered */
void sb_halo_exchange(sb_halo* h, double* x);
/* the same for a float vector (commExchange of the SP build): one plan serves either precision.  RCCL sends float32;
 * a host transport's neighbour_exchange carries the values widened to double, narrowed again into x[numRows ...] (exact) */
void sb_halo_exchange_f32(sb_halo* h, float* x);

/* ---- CG (solveCG, src/solver.h:11, src/CGSolver.c:62-141) --------------------- */
/* b_host / xexact_host: nr doubles in original row order (xexact may be NULL). */
sb_cg* sb_cg_create(const sb_matrix* m, sb_halo* halo, const double* b_host,
                    const double* xexact_host);
void sb_cg_free(sb_cg* s);
void sb_cg_debug_ptrs(const sb_cg* s, unsigned long long out[8]); /* lab: device addresses of r, p, p', Ap, x, b, partials, control block */
/* fused = 0: the reference's op list (waxpby, spMVM, ddot as separate launches); 1 (default): dots fused into the
 * SpMV / update kernels (5 launches per loop body, fewer with the folds below).  Same bits in both. */
void sb_cg_set_fused(sb_cg* s, int fused); /* every non-zero level is 1 (levels 2 and 3 were removed: DESIGN 4.6) */
/* The dot order of this solver's dots (r.r, p.Ap), src/solver.c:41-62: 0 = tree, 1 = seq (see sb_set_dot_order), -1 =
 * the process default (sb_dot_order; the initial setting).  seq runs the reference's op list (fused = 0: the region
 * table of sb_cg_region_ms is filled, sb_cg_launches_per_body is 0, sb_cg_fuse_p 0) with every dot as the sequential
 * sum: the history is the reference's solveCG history bit for bit.  The fused level set with sb_cg_set_fused is kept and
 * applies again under tree.  The order is latched by sb_cg_start for the whole solve; a change made between
 * sb_cg_start and sb_cg_finish takes effect with the next sb_cg_start.  sb_cg_dot_order: the order the solve
 * uses (or, outside a solve, will use). */
void sb_cg_set_dot_order(sb_cg* s, int order);
int sb_cg_dot_order(const sb_cg* s);
int sb_cg_vector_phase(sb_cg* s); /* always 0: the one-launch vector phase was removed */
/* launches per loop body the loop will use: 5 (p update | SpMV | alpha | r update | beta), 4 with the p update inside the
 * SpMV, one fewer for each scalar step folded into its consumer; 0 for the reference's op list.  Single precision: 3 on
 * Sell-64, 4 with the dot pass of CRS / generic C; on several ranks 7 / 8 on the peer-mapped plane (p update | push | pull |
 * SpMV | (dot pass) | alpha | r update | beta) and, on the communicator's, 5 / 6 + the pack (+ the unpack of a host
 * transport) + 2 */
int sb_cg_launches_per_body(sb_cg* s);
/* several ranks: the count above includes the halo kernels (peer-mapped push: +1, or +0 riding in the SpMV launch; pack
 * kernel in front of a send / recv group: +1) and, without the in-kernel all-reduce, one more kernel per dot (+2);
 * the communicator calls themselves (2 all-reduces, 1 send-recv group) are counted here: 0 on the peer-mapped paths */
int sb_cg_collectives_per_body(sb_cg* s);
/* The p update INSIDE the SpMV (round 3; pack.hip.h: spmv_prog_fusep): p = r + beta p (src/CGSolver.c:114; k = 1: p = r,
 * :109), the x update the previous body owes (:127) and Ap = A p with its p.Ap values (:123-125) as ONE launch -- every tile
 * forms p_new for its x window while it stages it and stores p_new / x for its own rows; p is double-buffered; on several
 * ranks the halo push forms the boundary values itself.  4 launches per body instead of 5; element for element the same
 * arithmetic in the same order: same bits.  Used where every chunk of the matrix is a masked row program with a mapped or
 * simple window, in the default loop (fused = 1), on one rank or with the peer-mapped halo; otherwise the separate p update.
 * on = 1 / 0 selects / deselects it, -1 = default (SB_FUSE_P, else the library's choice).  sb_cg_fuse_p: what the loop will do. */
void sb_cg_set_fuse_p(sb_cg* s, int on);
int sb_cg_fuse_p(sb_cg* s);
/* 1: the next solve of this solver runs the folded body of sb_comm_halo_fold (sb_cg_launches_per_body then counts 5),
 * 0: today's body.  Decided once per solve (sb_cg_start), like the fused p update and the dot order. */
int sb_cg_halo_fold(sb_cg* s);
/* The alpha step (src/CGSolver.c:124-126) inside the r update's launch: every workgroup of the r update reduces the p.Ap
 * values itself in the canonical order (identical bits everywhere), workgroup 0 records the step -- one launch fewer per loop
 * body on one rank (sb_cg_launches_per_body tells).  on = 1 / 0, -1 = default (SB_FUSE_ALPHA, else on).  Same bits. */
void sb_cg_set_fuse_alpha(sb_cg* s, int on);
/* The beta step / loop test (src/CGSolver.c:107, :111-113, :116) at the head of the next body's p update, where that is a launch
 * of its own (not inside the SpMV): taken by every workgroup, recorded by workgroup 0.  One rank: each workgroup reduces the r.r
 * values itself; several ranks on the communicator's collectives: the all-reduced sum is read, the third launch of the dot goes
 * (as for alpha: sb_cg_set_fuse_alpha).  Every sb_cg_run_iters call still leaves the loop state complete (a step left owing at
 * its end is taken by a launch of its own).  on = 1 / 0, -1 = default (SB_FUSE_BETA, else on).  Same bits. */
void sb_cg_set_fuse_beta(sb_cg* s, int on);
void sb_cg_set_graph(sb_cg* s, int use_graph); /* accepts and ignores use_graph: hipGraph replay was removed */
/* Runs solveCG's whole loop without host synchronisation; returns k exactly as
 * the reference does (src/CGSolver.c:140).  Blocking. */
int sb_cg_solve(sb_cg* s, int itermax, double eps);
/* The same in three steps, for callers that time a slice of the loop (bench.py):
 *   sb_cg_start      x0 = 0, prologue (src/CGSolver.c:94-103), loop test for k = 1; enqueues only
 *   sb_cg_run_iters  enqueue the next `iters` loop bodies (k = 1, 2, ...); never touches the host;
 *                    bodies past the reference's loop exit (k >= itermax or normr <= eps) are no-ops
 *   sb_cg_finish     wait and return k as solveCG does                                        */
void sb_cg_start(sb_cg* s, int itermax, double eps);
void sb_cg_run_iters(sb_cg* s, int iters);
int sb_cg_finish(sb_cg* s);
/* every r.r (index 0 = prologue) and p.Ap the solve produced, full precision */
int sb_cg_history(const sb_cg* s, double* rr_out, int rr_cap, double* pAp_out, int pAp_cap,
                  int* n_pAp);
void sb_cg_solution(const sb_cg* s, double* x_host); /* original row order */
double sb_cg_check_residual(const sb_cg* s);         /* max|x-xexact|, src/CGSolver.c:40-60 */
/* per-region milliseconds of the last unfused solve: [waxpby, spMVM, ddot, comm]
 * (regions of src/profiler.h:24) */
void sb_cg_region_ms(const sb_cg* s, double out[4]);
/* milliseconds the last solve's loop (k = 1 .. itermax-1) took on the GPU: what the
 * reference brackets with timeStart/timeStop (src/CGSolver.c:106,130) */
double sb_cg_loop_ms(const sb_cg* s);

/* bench instrumentation: bracket every SpMV launch of the loop with HIP events on the
 * layer's stream; sb_cg_spmv_ms returns their summed duration and count */
void sb_cg_spmv_timing(sb_cg* s, int on);
double sb_cg_spmv_ms(sb_cg* s, int* launches);
/* lab call: the same launches one by one (microseconds each); returns their number, writes at most cap */
int sb_cg_spmv_us_series(sb_cg* s, float* out, int cap);
/* per-kernel breakdown of the loop: an event after every launch of a loop body.  sb_cg_phase_ms returns the number
 * of phases P <= 8 and fills ms_out[i] / count_out[i] (summed milliseconds, occurrences) since timing was switched on:
 * 0 p update (+ owed x update), 1 halo (push kernel, or pack + send/recv), 2 SpMV (+ fused p.Ap partials; with the
 * peer-mapped halo: incl. the wait for the neighbours' pushes), 3 alpha step (levels 1-2 of p.Ap [+ all-reduce] +
 * alpha), 4 r update (+ r.r partials), 5 beta step / loop test (levels 1-2 of r.r [+ all-reduce] + beta),
 * 6 separate dot passes (reference op list, native CRS).  Every event costs ~1 us: never on in a clean timing. */
void sb_cg_phase_timing(sb_cg* s, int on);
int sb_cg_phase_ms(sb_cg* s, double ms_out[8], int count_out[8]);
/* device control block: out = {stop, stop_next, iters, n_rr, n_pAp} (proof that the
 * timed iterations really ran) */
void sb_cg_counters(const sb_cg* s, int out[5]);
/* Blocking test entries: the loop's double-precision vector and scalar kernels alone, through the launch functions the loop
 * uses.  Vectors, level-1 arrays, partials and histories are device pointers of the caller's (vectors 16-byte aligned); the
 * layer's stream; synchronised before return.  The control block is plain host data in the order of the device's block,
 * blk_d[9] = {rr, rr_old, pAp, alpha, beta, neg_alpha, local, eps, snap_rr} and blk_i[11] = {stop, stop_next, iters, n_rr,
 * n_pAp, itermax, hist_cap, x_pending, p2p_error, snap_iters, snap_stop_next}: uploaded between guard words, handed to the
 * kernel (its stop flag is the block's), and every field copied back into blk_d / blk_i; none is computed by the entry.
 * Each returns the number of guard words around the device's block that changed (0 unless a kernel wrote outside it).
 * sb_cg_update_p_native: mode 0 p = r + beta p (which != 0: r + 0.0 r) with, x_dev != NULL, which == 0 and x_pending, the
 * owed x += alpha p on the old p; mode 1 / 2 (which == 0): with the beta step and loop test at its head, r.r from the m
 * level-1 values l1_dev / from `local`, recorded into rr_hist_dev (hist_cap entries).
 * sb_cg_update_r_native: mode 0 r += neg_alpha Ap; mode 1 / 2: with the alpha step at its head, p.Ap from the m level-1
 * values l1in_dev / from `local`, recorded into pAp_hist_dev; the ceil(n/256) level-1 values of r.r go to l1out_dev.
 * sb_cg_scalar_native: the scalar step `mode` (0 prologue, 1 beta / loop test, 2 alpha) as its own launch; reduce != 0: the
 * sum of the m values q_dev (l1 != 0: level-1 values, else 4 m level-0 partials; to_local != 0: into `local`, no step),
 * reduce == 0: the sum is `local`.
 * sb_cg_x_finalize_native: x += alpha p where x_pending, p = p1_dev for an odd n_pAp, else p0_dev.
 * sb_cg_dot_spans_native: op 1 x += alpha a, r -= alpha b, op 2 r = a - b; the 4 ceil(n/256) level-0 partials of r.r.
 * sb_waxpby_sdev_native: w = x + alpha y (negative != 0: neg_alpha), the scalar read from the device's block. */
int sb_cg_update_p_native(int mode, uint32_t n, const double* r_dev, double* p_dev, double* x_dev, int which, uint32_t m,
    const double* l1_dev, double* rr_hist_dev, double* blk_d, int* blk_i);
int sb_cg_update_r_native(int mode, uint32_t n, const double* Ap_dev, double* r_dev, double* l1out_dev, uint32_t m,
    const double* l1in_dev, double* rr_hist_dev, double* pAp_hist_dev, double* blk_d, int* blk_i);
int sb_cg_scalar_native(int mode, int reduce, uint32_t m, const double* q_dev, double* rr_hist_dev, double* pAp_hist_dev,
    int to_local, int defer_x, int l1, double* blk_d, int* blk_i);
int sb_cg_x_finalize_native(uint32_t n, double* x_dev, const double* p0_dev, const double* p1_dev, double* blk_d, int* blk_i);
int sb_cg_dot_spans_native(int op, uint32_t n, const double* a_dev, const double* b_dev, double* x_dev, double* r_dev,
    double* partials_dev, double* blk_d, int* blk_i);
int sb_waxpby_sdev_native(uint32_t n, const double* x_dev, int negative, const double* y_dev, double* w_dev, double* blk_d,
    int* blk_i);
/* the launches of the two streaming kernels over n rows: out = {workgroups, threads per workgroup, CUs}; mode as above */
void sb_cg_update_p_launch(uint32_t n, uint32_t out[3]);
void sb_cg_update_r_launch(uint32_t n, int mode, uint32_t out[3]);

/* ---- the same for the single-precision loop ----
 * Blocking, one rank, through the launch functions the SP loop itself uses; device pointers of the caller's (vectors 16-byte
 * aligned), the layer's stream, synchronised before return.  The control block is plain host data,
 * blk_f[7] = {rr, rr_old, pAp, alpha, neg_alpha, eps, snap_rr}, blk_beta[1] (the double that carries the float quotient) and
 * blk_i[10] = {stop, stop_next, iters, n_rr, n_pAp, itermax, hist_cap, x_pending, snap_iters, snap_stop_next}: uploaded between
 * guard words, handed to the kernel, every field copied back; none is computed by the entry.  Each returns the number of guard
 * words around what it uploaded that changed (0 unless a kernel wrote outside it).
 * sb_cg_update_p_native_f32: mode 0 p = r + beta p (which != 0: r + 0.0 r) with, x_dev != NULL, which == 0 and x_pending, the
 * owed x += alpha p on the old p; mode 1 (which == 0): with the beta step and loop test at its head, r.r from the m level-1
 * values l1_dev, recorded into rr_hist_dev (hist_cap entries); launched at n = 0 too.
 * sb_cg_update_r_native_f32: mode 0 r += neg_alpha Ap unless the block's stop flag is set; mode 1: with the alpha step at its
 * head, p.Ap from the m level-1 values l1in_dev, recorded into pAp_hist_dev; the ceil(n/256) level-1 values of r.r to l1out_dev.
 * sb_cg_scalar_native_f32: the scalar step `mode` (0 prologue, 1 beta / loop test, 2 alpha) on the sum of the m values q_dev
 * (l1 != 0: level-1 values, else 4 m level-0 partials).  split 0: one launch; split 1: the sum alone (cg_local_f32_k) into
 * *local, which keeps its value on a set stop flag; split 2: the step alone on the given *local (q_dev, m and l1 unused).
 * sb_cg_x_finalize_native_f32: x += alpha p where x_pending; p1_dev == NULL: p = p0_dev, else p = p1_dev for an odd n_pAp.
 * sb_axpy_sdev_native_f32: w = x + alpha y (negative != 0: neg_alpha), scalar and stop flag read from the device's block.
 * sb_dot_l1_native_f32: the ceil(n/256) level-1 values of a . b; sb_waxpby_stop_native_f32: sb_waxpby_f32; both with a stop flag
 * of their own on the device that holds `stopped`. */
int sb_cg_update_p_native_f32(int mode, uint32_t n, const float* r_dev, float* p_dev, float* x_dev, int which, uint32_t m,
    const float* l1_dev, float* rr_hist_dev, float* blk_f, double* blk_beta, int* blk_i);
int sb_cg_update_r_native_f32(int mode, uint32_t n, const float* Ap_dev, float* r_dev, float* l1out_dev, uint32_t m,
    const float* l1in_dev, float* rr_hist_dev, float* pAp_hist_dev, float* blk_f, double* blk_beta, int* blk_i);
int sb_cg_scalar_native_f32(int mode, int split, uint32_t m, const float* q_dev, float* rr_hist_dev, float* pAp_hist_dev,
    int defer_x, int l1, float* blk_f, double* blk_beta, int* blk_i, float* local);
int sb_cg_x_finalize_native_f32(uint32_t n, float* x_dev, const float* p0_dev, const float* p1_dev, float* blk_f,
    double* blk_beta, int* blk_i);
int sb_axpy_sdev_native_f32(uint32_t n, const float* x_dev, int negative, const float* y_dev, float* w_dev, float* blk_f,
    double* blk_beta, int* blk_i);
int sb_dot_l1_native_f32(uint32_t n, const float* a_dev, const float* b_dev, float* l1out_dev, int stopped);
int sb_waxpby_stop_native_f32(uint32_t n, float alpha, const float* x_dev, float beta, const float* y_dev, float* w_dev,
    int stopped);
/* their launches over n rows: out = {workgroups, threads per workgroup, CUs}; sb_stream_launch_f32: the 256-thread kernels'
 * (axpy_sdev, waxpby, both x finalizes) */
void sb_cg_update_p_launch_f32(uint32_t n, uint32_t out[3]);
void sb_cg_update_r_launch_f32(uint32_t n, uint32_t out[3]);
void sb_dot_l1_launch_f32(uint32_t n, uint32_t out[3]);
void sb_stream_launch_f32(uint32_t n, uint32_t out[3]);

/* ---- restarted GMRES(m) (the solver the reference's driver names and leaves empty: src/main.c:31,217-222) ------ */
/* For matrices that are not symmetric positive definite.  Double precision, ONE rank; a single-precision matrix, several
 * ranks or restart < 1 are fatal errors with file:line.  The numerical contract is DESIGN 4.8: x0 = 0, b / xexact as
 * sb_cg_create takes them, classical Gram-Schmidt with one reorthogonalisation (CGS2), every dot the tree order of sb_ddot
 * over the device's row order, Givens rotations, the iteration counter and loop test of solveCG (src/CGSolver.c:105-107,140:
 * k starts at 1, the loop runs while k < itermax && normr > eps on the residual ESTIMATE, k is returned).  The loop is
 * device-resident like CG's: a control block in HBM, every kernel returns at once when its stop flag is set.
 * b_host / xexact_host: nr doubles in original row order (xexact may be NULL); halo: NULL (one rank). */
sb_gmres* sb_gmres_create(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int restart);
void sb_gmres_free(sb_gmres* s);
/* 1 (default): the fused kernels (multi-dot, multi-update); 0: the op list -- sb_spmv_native, one tree dot per h entry, one
 * waxpby-shaped launch per projection (w = 1.0*w + (-h)*V[i] is bit-identical to w - h*V[i]), a divide-by-scalar.  Same bits
 * in both.  Not between sb_gmres_start and sb_gmres_finish. */
void sb_gmres_set_fused(sb_gmres* s, int fused);
int sb_gmres_restart(const sb_gmres* s);
/* launches of the Arnoldi step at cycle position j (0-based): 7, + 1 at j = 0 (the cycle's first basis vector), + 5 at
 * j = restart - 1 (the cycle close); 0 for the op list */
int sb_gmres_launches_per_step(sb_gmres* s, int j);
int sb_gmres_solve(sb_gmres* s, int itermax, double eps); /* blocking; returns k */
/* The same in three steps: sb_gmres_start x0 = 0, r = b - A x, r.r, the loop test for k = 1 (enqueues only);
 * sb_gmres_run_steps enqueues the next `steps` Arnoldi steps (with the cycle closes between them), never touches the host,
 * steps past the loop's exit are no-ops; sb_gmres_finish waits, closes the cycle the exit left open (x takes its columns,
 * r.r of the final x is recorded) and returns k. */
void sb_gmres_start(sb_gmres* s, int itermax, double eps);
void sb_gmres_run_steps(sb_gmres* s, int steps);
int sb_gmres_finish(sb_gmres* s);
/* res_out[k]: the residual estimate after the step taken at counter k (res_out[0]: the initial norm); rr_out: the explicit
 * r.r of the prologue and of every cycle close, the last one included.  Returns the number of estimates. */
int sb_gmres_history(const sb_gmres* s, double* res_out, int res_cap, double* rr_out, int rr_cap, int* n_rr);
void sb_gmres_solution(const sb_gmres* s, double* x_host); /* original row order */
double sb_gmres_check_residual(const sb_gmres* s);         /* max|x - xexact| */
double sb_gmres_loop_ms(const sb_gmres* s); /* GPU milliseconds between the end of sb_gmres_start and sb_gmres_finish */
void sb_gmres_counters(const sb_gmres* s, int out[5]); /* {stop, steps run, cycles closed, n_res, n_rr} */
/* the two vector kernels on their own, for parity tests and for callers that orthogonalise blocks themselves:
 * V = nvec vectors of n doubles, vector i at V + i*ldv (ldv >= n, a multiple of 2; V and w 16-byte aligned).
 * sb_multidot: h[i] = tree dot of V[i] and w, all from one read of w.  sb_multiaxpy_sub: w[e] = (..(w[e] - h[0]*V[0][e]) ..
 * - h[nvec-1]*V[nvec-1][e]), ascending i, every product rounded before its subtraction.  Stream-ordered. */
void sb_multidot(uint32_t n, int nvec, const double* V, size_t ldv, const double* w, double* h_dev);
void sb_multiaxpy_sub(uint32_t n, int nvec, const double* V, size_t ldv, const double* h_dev, double* w);
/* their launch over n rows: out = {workgroups, threads per workgroup, CUs} */
void sb_gmres_group_launch(uint32_t n, uint32_t out[3]);
/* the launch of the scale kernels (256 threads a workgroup, a row per thread and trip) and of the step-and-normalise kernels
 * (min(CUs, ceil(n / 4096)) workgroups of 1 024 threads) over n rows: out = {workgroups, threads per workgroup, CUs} */
void sb_gmres_scale_launch(uint32_t n, uint32_t out[3]);
void sb_gmres_step_launch(uint32_t n, uint32_t out[3]);
/* Test entries (blocking): every kernel of the GMRES loop alone on the caller's buffers, launched by the loop's own launch
 * functions.  Each returns the number of guard words around its control block that the launch changed (0).
 * Entries whose kernel reads a stop flag and nothing else of the block take `stopped`: the flag's value.  Entries whose kernel
 * reads or writes the block take it as plain data,
 *   blk_d[4] = {normr, eps, hn, rr}
 *   blk_i[9] = {stop, k, j, itermax, n_res, n_rr, hist_cap, cycles, steps}
 * in and out; use_stop: the launch is handed the block's own stop flag (1) or none (0).  dense_host, in and out: the dense
 * state of a cycle of restart length m as the handle lays it out, m (m + 1) + 3 m + 6 (m + 1) doubles: H (column j at
 * j (m + 1)), cs, sn, y (m each), g, h1, h2, nh1, nh2, hcol (m + 1 each).  V, ldv, mode, c1, dinv, d, z as in
 * sb_multidot and the sb_gmres_pre_*_native entries.
 * multidot: l1_dev[i nGroups + group] = level-1 value of dot(V[i], w), nGroups = (n + 255) / 256.
 * finish_dots: workgroup i of nvec finishes dot i from q_dev + i qStride (l1 != 0: nGroups level-1 values, 0: 4 nGroups level-0
 *   partials): out[i], nout[i] = -out[i], sum[i] = add[i] + out[i]; nout_dev, add_dev and sum_dev may be NULL.
 * project: w -= c[i] V[i], ascending i; epi 1: l1_dev[group] of w . w, epi 2: l1_dev[i nGroups + group] of dot(V[i], w).
 * multiadd, scale: sb_gmres_pre_multiupdate_native and sb_gmres_pre_scale_native with a stop flag (g0_dev may be NULL).
 * rr: gm_rr_k<mode> (0 the prologue, 1 a close inside the loop, 2 the close of sb_gmres_finish) over nGroups values at q_dev.
 * step: the scalar step at cycle position j.  scale 0: the op list's kernel over nGroups values at q_dev (l1 as in
 *   finish_dots), mode -1.  scale 1: q_dev holds the (n + 255) / 256 level-1 values of w . w, vnext = w / hn and the first part
 *   of M^-1 of it ride.  The kernel reads the block's stop flag itself.
 * backsolve: y[0 .. nvec-1] of the dense state from g and H's first nvec columns. */
int sb_gmres_multidot_native(uint32_t n, int nvec, const double* V_dev, size_t ldv, const double* w_dev, double* l1_dev, int stopped);
int sb_gmres_finish_dots_native(uint32_t nGroups, int nvec, const double* q_dev, size_t qStride, int l1, double* out_dev, double* nout_dev,
    const double* add_dev, double* sum_dev, int stopped);
int sb_gmres_project_native(int epi, uint32_t n, int nvec, const double* V_dev, size_t ldv, const double* c_dev, double* w_dev, double* l1_dev,
    int stopped);
int sb_gmres_multiadd_native(uint32_t n, int mode, double c1, int nvec, const double* V_dev, size_t ldv, const double* c_dev, double* w_dev,
    const double* dinv_dev, double* d_dev, double* z_dev, int stopped);
int sb_gmres_scale_native(uint32_t n, int mode, double c1, const double* a_dev, const double* scalar_dev, double* out_dev, double* g0_dev,
    const double* dinv_dev, double* d_dev, double* z_dev, int stopped);
int sb_gmres_rr_native(int mode, uint32_t nGroups, const double* q_dev, int l1, double* res_hist_dev, double* rr_hist_dev, int use_stop,
    double* blk_d, int* blk_i);
int sb_gmres_step_native(int scale, int mode, double c1, uint32_t n, int j, int m, uint32_t nGroups, const double* q_dev, int l1,
    const double* w_dev, double* vnext_dev, const double* dinv_dev, double* d_dev, double* z_dev, double* res_hist_dev, double* blk_d, int* blk_i,
    double* dense_host);
int sb_gmres_backsolve_native(int m, int nvec, int use_stop, double* blk_d, int* blk_i, double* dense_host);
/* test entry: sqrt_dev[e] = sqrt(a[e]), div_dev[e] = a[e] / b[e] as the scalar steps compute them (IEEE correctly rounded) */
void sb_debug_sqrt_div(uint32_t n, const double* a_dev, const double* b_dev, double* sqrt_dev, double* div_dev);

/* ---- batched CG: nrhs right-hand sides on one pass over the matrix ----------------------------------- */
/* nrhs INDEPENDENT CG solves (not block CG: every column has its own alpha, beta, residual, loop test and iteration count)
 * whose loop bodies share one stream of the matrix.  The contract is exact: column c is bit for bit sb_cg_create(..., b_c, ...)
 * solved alone in the tree dot order -- k_c, every r.r, every p.Ap, x_c.  Double precision, ONE rank, tree order, nrhs in
 * {2, 4, 8}; anything else (another width, a halo with more than one rank, a single-precision matrix, the seq order) is a
 * fatal error with file:line.  The batched path streams the reference layout whatever sb_matrix_use_packed selected: the
 * compressed mirror and the row programs take one vector.  Only Sell-C-sigma with C = 64 is tuned; CRS and other C run a
 * one-thread-per-row correctness kernel.
 * A BLOCK VECTOR is interleaved, element (row, c) at X[row * nrhs + c], rows in the device's row order (the permuted order
 * for sigma > 1), 16-byte aligned. */
typedef struct sb_cgb sb_cgb;
/* Y = A X on block vectors (device pointers; X has nc rows, Y nr). */
void sb_spmmv_native(const sb_matrix* m, int nrhs, const double* X_dev, double* Y_dev);
/* ... with the fused level-1 values of X_c . Y_c, column c at l1_dev + c * ceil(nr/256): what the batched loop launches for
 * p . Ap.  Returns 2 (level-1 values, as sb_spmv_native_dot does), or 0 without having run where the block kernel has no
 * fused dot (CRS, C != 64). */
int sb_spmmv_native_dot(const sb_matrix* m, int nrhs, const double* X_dev, double* Y_dev, double* l1_dev);
/* nrhs plain vectors of nr doubles in ORIGINAL row order (vector c at cols_dev + c * nr) -> one block vector of nr rows, and
 * back; both permute for sigma > 1.  Device pointers, stream-ordered. */
void sb_block_interleave(const sb_matrix* m, int nrhs, const double* cols_dev, double* X_dev);
void sb_block_deinterleave(const sb_matrix* m, int nrhs, const double* X_dev, double* cols_dev);
/* algorithmic bytes of one SpMMV: the matrix part of sb_matrix_spmv_bytes once + nrhs times its vector part */
double sb_matrix_spmmv_bytes(const sb_matrix* m, int nrhs);
/* B_host: nrhs vectors of nr doubles in original row order, vector c at B_host + c * nr.  xexact0_host: the exact solution of
 * column 0 (nr doubles) or NULL -- the other columns have none.  halo: NULL or a one-rank plan. */
sb_cgb* sb_cgb_create(const sb_matrix* m, sb_halo* halo, int nrhs, const double* B_host, const double* xexact0_host);
void sb_cgb_free(sb_cgb* s);
int sb_cgb_nrhs(const sb_cgb* s);
/* 5 on Sell-64 (p update | SpMMV with the p.Ap values | alpha steps | r update with the r.r values | beta steps; a scalar
 * step is one launch of nrhs workgroups); 6 where the block kernel has no fused dot (+ the dot pass) */
int sb_cgb_launches_per_body(const sb_cgb* s);
int sb_cgb_solve(sb_cgb* s, int itermax, double eps); /* blocking; returns the largest k_c */
/* The same in three steps, as sb_cg_start / _run_iters / _finish: bodies enqueued past every column's exit are no-ops, a
 * column that has stopped no longer changes (the SpMMV still computes it), nothing is read back between bodies. */
void sb_cgb_start(sb_cgb* s, int itermax, double eps);
void sb_cgb_run_iters(sb_cgb* s, int iters);
int sb_cgb_finish(sb_cgb* s);
int sb_cgb_iterations(const sb_cgb* s, int c); /* k_c */
int sb_cgb_history(const sb_cgb* s, int c, double* rr_out, int rr_cap, double* pAp_out, int pAp_cap, int* n_pAp);
void sb_cgb_solution(const sb_cgb* s, int c, double* x_host); /* x_c, original row order */
double sb_cgb_check_residual(const sb_cgb* s, int c);         /* max|x_0 - xexact_0| for c = 0 with an exact solution, else 0.0 */
double sb_cgb_loop_ms(const sb_cgb* s); /* GPU milliseconds between the end of sb_cgb_start and sb_cgb_finish */
/* c >= 0: {stop, stop_next, iters, n_rr, n_pAp} of column c; c = -1: {all stopped, columns stopped, bodies enqueued, 0, 0} */
void sb_cgb_counters(const sb_cgb* s, int c, int out[5]);
/* Blocking test entries: the loop's vector kernels alone, through the launch functions the loop uses.  Block vectors of n rows
 * (device pointers, 16-byte aligned); neg_alpha / beta / alpha / stop / x_pending: nrhs HOST values, column c's at [c], put into
 * zeroed control blocks; the global stop flag is clear.
 * sb_block_vec_native, op 0: l1 = level-1 values of A_c . B_c.  op 1: R_c += neg_alpha_c * A_c and the level-1 values of
 * R_c . R_c; a column with stop_c != 0 keeps its R_c and its l1 values (B_dev unused).  op 2: R_c = A_c + (-1.0) * B_c and the
 * level-1 values of R_c . R_c (ops 0 and 2 read neither host array).  Column c's ceil(n/256) values at l1_dev + c * ceil(n/256).
 * sb_cgb_update_p_native: P_c = R_c + beta_c * P_c (which != 0: R_c + 0.0 * R_c; beta and x_pending unused) after, where
 * x_pending_c != 0 and which == 0, X_c += alpha_c * P_c on the old P_c; a column with stop_c != 0 keeps P_c and X_c.
 * sb_cgb_x_finalize_native: X_c += alpha_c * P_c where x_pending_c != 0. */
void sb_block_vec_native(int op, int nrhs, uint32_t n, const double* A_dev, const double* B_dev, double* R_dev,
    const double* neg_alpha_host, const int* stop_host, double* l1_dev);
void sb_cgb_update_p_native(int nrhs, uint32_t n, const double* R_dev, double* P_dev, double* X_dev, const double* beta_host,
    const double* alpha_host, const int* stop_host, const int* x_pending_host, int which);
void sb_cgb_x_finalize_native(int nrhs, uint32_t n, double* X_dev, const double* P_dev, const double* alpha_host,
    const int* x_pending_host);
/* their launches over n rows: out = {workgroups, threads per workgroup, CUs}; sb_block_vec_launch: sb_block_vec_native's,
 * sb_cgb_rows_launch: the other two's */
void sb_block_vec_launch(uint32_t n, uint32_t out[3]);
void sb_cgb_rows_launch(uint32_t n, uint32_t out[3]);

/* ---- CG with a diagonal preconditioner ---------------------------------------------------------------- */
/* solveCG's loop with z = r o dinv put back (HPCG's CG with its preconditioner): alpha = r.z / p.Ap, beta = r.z / (r.z)_old,
 * p = z + beta p; the loop test stays on sqrt(r.r) with solveCG's one-body lag, so dinv = 1.0 everywhere is sb_cg in the tree
 * order bit for bit (k, every r.r, every p.Ap, x; r.z == r.r).  Double precision, tree dot order; a single-precision matrix, the
 * seq order, a matrix row without a finite positive diagonal (Jacobi) and a caller's dinv entry that is not finite and positive
 * are fatal errors with file:line.  The SpMV is the one the matrix's kernel mode selects (sb_matrix_use_packed), as
 * sb_spmv_native_dot launches it.
 * ONE rank -- or, for sb_pcg_create and sb_pcg_create_poly alone, SEVERAL: the process is in a communicator of more
 * than one rank and `halo` is the plan of this matrix (halo->nr == nr, nr + externalCount == nc; a plan that disagrees is a fatal
 * error).  Then every call on the handle from create to free is collective, as sb_cg's are.  Each of p.Ap, r.z and r.r is the
 * rank's own tree-order value, then the pairwise tree over ranks in rank order (sb_cg's all-reduce; r.z and r.r travel back to
 * back); p's halo tail is filled ahead of every SpMV by the plan's push and pull launches or by pack | send / recv, never by a
 * folded form: sb_comm_halo_fold and sb_comm_halo_push_inside do not apply to PCG.  Same bits on either data plane and as the
 * P-rank restatement of the tests.  A failed wait on the peer-mapped plane ends the process in sb_pcg_finish with sb_cg's
 * messages.  In every other case with halo columns, a halo plan of another rank count or several ranks the handles are refused:
 * "PCG runs on one rank", as are the sweeps and the V-cycles (below), and a BiCGStab or GMRES handle that borrows a several-rank
 * handle's preconditioner. */
typedef struct sb_pcg sb_pcg;
/* d_dev[i] = the sum, in storage order from +0.0, of row i's stored entries whose column is i; device pointer, nr doubles,
 * the device's row order (the permuted order for sigma > 1); stream-ordered */
void sb_matrix_diagonal(const sb_matrix* m, double* d_dev);
/* b_host, xexact_host (or NULL) as for sb_cg_create.  dinv_host NULL: Jacobi, dinv_i = 1.0 / d_i of the rank's own rows; else nr
 * finite positive doubles in ORIGINAL row order (the rank's nr local entries).  halo: NULL or a one-rank plan; several ranks: the
 * matrix's plan. */
sb_pcg* sb_pcg_create(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, const double* dinv_host);
void sb_pcg_free(sb_pcg* s);
int sb_pcg_solve(sb_pcg* s, int itermax, double eps); /* blocking; returns k as solveCG does */
/* The same in three steps, as sb_cg_start / _run_iters / _finish: bodies enqueued past the exit are no-ops, nothing is read
 * back between bodies; a handle can be solved again. */
void sb_pcg_start(sb_pcg* s, int itermax, double eps);
void sb_pcg_run_iters(sb_pcg* s, int iters);
int sb_pcg_finish(sb_pcg* s);
/* rr[0], rz[0]: the prologue's; then one rr, one rz (both under rr_cap / rz_cap, the smaller counts) and one pAp per body, as
 * sb_cg_history indexes its own.  Returns the number of rr (= rz) entries. */
int sb_pcg_history(const sb_pcg* s, double* rr_out, int rr_cap, double* rz_out, int rz_cap, double* pAp_out, int pAp_cap, int* n_pAp);
void sb_pcg_solution(const sb_pcg* s, double* x_host);   /* original row order */
double sb_pcg_check_residual(const sb_pcg* s);           /* max|x - xexact| (several ranks: over all of them), 0.0 without an exact solution */
void sb_pcg_dinv(const sb_pcg* s, double* dinv_host);    /* the preconditioner in use, original row order */
/* 5 (p update | SpMV with the p.Ap values | alpha | r update with z and the r.z, r.r values | beta); 6 where the selected SpMV
 * kernel has no fused dot (native CRS, C != 64: + the dot pass).  Several ranks add, as sb_cg_launches_per_body counts them: per
 * halo exchange (one for p; the polynomial: one more per step behind the first) the push and the pull kernel on the peer-mapped
 * plane, else the pack kernel; and 2 without the in-kernel all-reduce (local reduce | all-reduces | step, for alpha and for beta) */
int sb_pcg_launches_per_body(const sb_pcg* s);
/* communicator calls per body, as sb_cg_collectives_per_body: 3 all-reduces (p.Ap; r.z, r.r) without the in-kernel all-reduce, a
 * send / recv group per halo exchange without the peer-mapped halo; 0 on one rank */
int sb_pcg_collectives_per_body(const sb_pcg* s);
double sb_pcg_loop_ms(const sb_pcg* s); /* GPU milliseconds between the end of sb_pcg_start and sb_pcg_finish */
void sb_pcg_counters(const sb_pcg* s, int out[5]); /* stop, stop_next, iters, n_rr, n_pAp of the device control block */
/* test entry for the fused kernel: r = r + nalpha * Ap, z = r o dinv and the ceil(n/256) level-1 values of r.z and of r.r;
 * r, Ap, dinv, z device vectors of n doubles (16-byte aligned), nalpha a host scalar; blocking */
void sb_pcg_update_r_native(uint32_t n, double nalpha, const double* Ap_dev, double* r_dev, const double* dinv_dev, double* z_dev,
                            double* l1_rz_dev, double* l1_rr_dev);
/* its launch over n rows: {workgroups, threads per workgroup, compute units of the device}; a wave owns whole 256-row groups
 * and strides over them by the number of waves in the grid */
void sb_pcg_update_r_launch(uint32_t n, uint32_t out[3]);
/* test entry for the several-rank loop's local reduce on the communicator's plane (pcg_local_reduce_k), in one process: the
 * level-1 values of a.b and a.a over n rows (dot_l1_k), then the kernel; out: the block's two sums, preset to { -1.0, -2.0 }:
 * out[0] = levels 1-2 of a.b, out[1] = of a.a where two != 0 and untouched else; stopped != 0: the control block says the loop
 * has exited and both are untouched.  a, b: device vectors of n doubles, 16-byte aligned; blocking */
void sb_pcg_local_reduce_native(uint32_t n, int two, int stopped, const double* a_dev, const double* b_dev, double out[2]);

/* ---- symmetric Gauss-Seidel preconditioning by multicolouring ----
 * z = M^-1 r with M = (D + L) D^-1 (D + U) in a colour order: rows are adjacent when a_ij or a_ji is stored, off the diagonal
 * and non-zero; rows 0, 1, ... of the device's order each take the smallest colour no adjacent, already coloured row has.  A
 * colour is one launch: nC forward, nC - 1 backward per apply.  The handle is an sb_pcg: every other sb_pcg_* call works on it,
 * sb_pcg_dinv gives 1 / diag(A).  Square matrix, double precision, one rank, tree dot order; a row without a finite positive
 * diagonal is a fatal error.  The set-up downloads the matrix once and builds the sweep structure on the host. */
sb_pcg* sb_pcg_create_sgs(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host);
int sb_pcg_precond(const sb_pcg* s); /* 0 diagonal, 1 SGS, 2 MG, 3 MG with full-weighting transfers (below), 4 Chebyshev polynomial,
                                        5 Chebyshev-smoothed MG */
int sb_pcg_colours(const sb_pcg* s); /* nC; 0 for a diagonal handle */
void sb_pcg_colouring(const sb_pcg* s, uint32_t* colour_host); /* nr colours, original row order; SGS handles only */
/* z = M^-1 r once, with the handle's preconditioner (either kind), on host vectors of nr doubles in original row order;
 * blocking, on scratch vectors of its own; a fatal error between sb_pcg_start and sb_pcg_finish */
void sb_pcg_apply_precond(sb_pcg* s, const double* r_host, double* z_host);
/* GPU milliseconds per apply, the mean of `reps` back-to-back applies (after one untimed) on scratch vectors holding b; blocking;
 * not between sb_pcg_start and sb_pcg_finish */
double sb_pcg_apply_precond_ms(sb_pcg* s, int reps);
/* bytes one apply reads and writes: the sweep structure and the vector traffic (diagonal: 24 per row) */
double sb_pcg_precond_bytes(const sb_pcg* s);

/* ---- multigrid V-cycle preconditioning, HPCG's own ----
 * z = V(0, r) on levels 0 .. nCoarse (level 0 is m): pre-smooth from zero with the SGS apply above, the residual at the coarse
 * points only, the cycle on the next level, the correction added at the coarse points, post-smooth from that guess (forward over
 * all colours, backward over all but the last).  Injection: f2c_host[l] holds the coarse[l]->nr distinct rows of level l that are
 * level l + 1's points, both sides in original row numbering.  Every level: square, double precision, fewer rows than the one
 * above, a finite positive diagonal in every row; any format, its own permutation.  The caller keeps the coarse matrices alive
 * as it does m.  nCoarse = 0 is sb_pcg_create_sgs bit for bit.  One rank, tree dot order.  On the handle sb_pcg_colours and
 * sb_pcg_colouring report level 0, sb_pcg_launches_per_body counts the cycle, sb_pcg_precond_bytes sums the levels. */
sb_pcg* sb_pcg_create_mg(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int nCoarse,
    const sb_matrix* const* coarse, const uint32_t* const* f2c_host);
int sb_pcg_levels(const sb_pcg* s);                  /* L of an MG handle; 1 SGS; 0 diagonal */
uint32_t sb_pcg_level_rows(const sb_pcg* s, int l);  /* n_l */
int sb_pcg_level_colours(const sb_pcg* s, int l);    /* nC_l */

/* ---- the V-cycle with full-weighting transfers ----
 * sb_pcg_create_mg with a prolongation per level in the injection map's place: P_l = (p_ptr[l], p_col[l], p_val[l]) is CSR with
 * n_l rows and columns < n_{l+1}, original row numbering on both sides, 64-bit row pointers.  Between the two smoothings of level
 * l the cycle takes the FULL residual d = r - A z (one launch over all colours), restricts rc = omega[l] * (P_l^T d) -- a coarse
 * row's terms in ascending original fine row number -- and prolongs z = z + P_l zc, a row's terms in storage order; rows of P
 * without an entry are left alone and a stored weight of 0.0 is dropped.  Refused before anything is built, each naming the
 * level: what sb_pcg_create_mg refuses, a column out of range, a row pointer that falls, a weight that is not finite, an omega
 * that is not finite and positive.  nCoarse = 0 is sb_pcg_create_sgs bit for bit.  sb_pcg_precond gives 3; the level queries,
 * sb_pcg_launches_per_body (one more launch per level but the last) and sb_pcg_precond_bytes count this cycle. */
sb_pcg* sb_pcg_create_mg_p(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int nCoarse,
    const sb_matrix* const* coarse, const uint64_t* const* p_ptr, const uint32_t* const* p_col, const double* const* p_val,
    const double* omega);
/* test entry, blocking, on scratch vectors; refused between sb_pcg_start and sb_pcg_finish.  The transfers of level l alone
 * (l + 1 < levels): d_out = r - A_l z and rc_out = omega_l P_l^T d_out from (r, z), z_out = z + P_l zc.  r, z, d_out, z_out: n_l
 * doubles in level l's original row order; zc, rc_out: n_{l+1} doubles in level l + 1's */
void sb_pcg_mg_fw_probe(sb_pcg* s, int l, const double* r_host, const double* z_host, const double* zc_host, double* d_out,
    double* rc_out, double* z_out);

/* ---- Chebyshev polynomial preconditioning ----
 * z = q(D^-1 A) D^-1 r, `steps` terms of the Chebyshev recurrence for D^-1 A on [lmin, lmax], lmin = lmax / ratio.  Step 1:
 * d = z = (r o dinv) * c1.  Step j >= 2: w = A z by the matrix's selected SpMV (any kernel mode), then per row u = r - w,
 * u = u * dinv, d = (a_j * d) + (b_j * u), z = z + d.  Host doubles, in this order: theta = (lmax + lmin) * 0.5,
 * delta = (lmax - lmin) * 0.5, sigma = theta / delta, c1 = 1.0 / theta, rho_1 = 1.0 / sigma, rho_j = 1.0 / (2.0 * sigma - rho_{j-1}),
 * a_j = rho_j * rho_{j-1}, b_j = (2.0 * rho_j) / delta.  No colouring, no structure, no matrix download.
 * steps: 1 .. 16.  lmax <= 0.0: the bound max_i g_i, g_i the sum in storage order from +0.0 over row i's stored entries of
 * (|a_e| * sd_i) * sd[col_e], sd = sqrt(dinv): an absolute row sum of D^-1/2 A D^-1/2, computed on the device.  ratio == 0.0: 16.
 * Fatal errors: steps out of range, a ratio that is not finite and > 1, an lmax that is not finite, a bound that is not finite
 * and positive, and what sb_pcg_create refuses (a row without a finite positive diagonal names this preconditioner).
 * Several ranks (as sb_pcg_create accepts them): steps, lmax and ratio are COLLECTIVE arguments, the same on every rank; the bound
 * reads dinv at the halo columns (one halo exchange at set-up) and lmax is the MAX over ranks; z's halo tail is filled ahead of
 * every step's SpMV; a rank must receive from exactly the ranks it sends to (a structurally symmetric matrix), else fatal;
 * sb_pcg_poly_rowbound gives the rank's own rows, sb_pcg_apply_precond is collective.  The handle
 * is an sb_pcg: every other sb_pcg_* call works on it, sb_pcg_dinv gives 1 / diag(A), sb_pcg_launches_per_body gives
 * 5 + 2 (steps - 1) (+ 1 without a fused dot), sb_pcg_precond_bytes (steps - 1) * (sb_matrix_spmv_bytes + 56 per row) + 24 per row. */
sb_pcg* sb_pcg_create_poly(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int steps, double lmax,
    double ratio);
int sb_pcg_poly_steps(const sb_pcg* s);                     /* 0 for a handle of another kind */
void sb_pcg_poly_interval(const sb_pcg* s, double out[2]);  /* lmin, lmax */
void sb_pcg_poly_coeffs(const sb_pcg* s, double* out);      /* 2 steps - 1 doubles: c1, then a_j, b_j for j = 2 .. steps */
void sb_pcg_poly_rowbound(const sb_pcg* s, double* g_host); /* g, nr doubles, original row order */
/* test entries for the two streaming kernels, blocking; device vectors of n doubles (16-byte aligned), host scalars.
 * update_r: r = r + nalpha * Ap (pro: r = r + (-1.0) * Ap, the prologue's form), d = z = (r o dinv) * c1, the ceil(n/256) level-1
 * values of r.r and, with last, of r.z (l1_rz_dev is not touched otherwise).  step: one step j >= 2 from (r, w, dinv, d, z) with
 * coefficients a, b; with last the level-1 values of r.z */
void sb_pcg_poly_update_r_native(uint32_t n, int pro, int last, double nalpha, double c1, const double* Ap_dev, double* r_dev,
    const double* dinv_dev, double* d_dev, double* z_dev, double* l1_rz_dev, double* l1_rr_dev);
void sb_pcg_poly_step_native(uint32_t n, int last, double a, double b, const double* r_dev, const double* w_dev, const double* dinv_dev,
    double* d_dev, double* z_dev, double* l1_rz_dev);
/* their launch over n rows, as sb_pcg_update_r_launch reports its own */
void sb_pcg_poly_step_launch(uint32_t n, uint32_t out[3]);

/* ---- the V-cycle with the Chebyshev polynomial as its smoother ----
 * z = V(0, r) on levels 0 .. nCoarse with the hierarchy arguments of sb_pcg_create_mg_p.  V(l, r): z = the polynomial apply above
 * on level l from zero (`steps` steps; the last level `coarse_steps`, 0: as many as steps) and, unless l is the last level:
 * w = A_l z by the level's selected SpMV; rc_c = omega_l * s with s = +0.0 and s = s + w_e * (r[row_e] - w[row_e]) over row c of
 * P_l^T in ascending original fine row number (no residual vector is written); zc = V(l + 1, rc); z = z + P_l zc as
 * sb_pcg_create_mg_p prolongs; then `steps` steps from that guess: w = A_l z, per row u = r - w, u = u * dinv, d = u * c1,
 * z = z + d, and steps j >= 2 exactly as the polynomial's.  Per level dinv = 1 / diag, the interval [lmax_l / ratio, lmax_l] with
 * lmax_l the row-sum bound of that level's matrix (lmax <= 0.0) or the caller's lmax on every level, and the coefficients by the
 * formulas above.  ratio == 0.0: 4.  No colouring, no matrix download: sb_pcg_colours gives 0.  Fatal errors, by name and level:
 * what sb_pcg_create_mg_p and sb_pcg_create_poly refuse.  nCoarse = 0 is sb_pcg_create_poly with coarse_steps steps bit for bit.
 * sb_pcg_precond gives 5, sb_pcg_poly_steps `steps`; the level queries work; sb_pcg_launches_per_body gives
 * 4 + nCoarse * (4 steps + 2) + 2 coarse_steps - 1 (+ 1 without a fused dot); sb_pcg_precond_bytes per level but the last
 * 2 steps * sb_matrix_spmv_bytes + (2 (steps - 1) * 56 + 48 + 24) per row + both transfer structures + 32 per row + 16 per coarse
 * row, the last level as the polynomial's. */
sb_pcg* sb_pcg_create_mg_poly(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int nCoarse,
    const sb_matrix* const* coarse, const uint64_t* const* p_ptr, const uint32_t* const* p_col, const double* const* p_val,
    const double* omega, int steps, int coarse_steps, double lmax, double ratio);
int sb_pcg_mg_poly_level_steps(const sb_pcg* s, int l);               /* steps; on the last level coarse_steps */
void sb_pcg_mg_poly_interval(const sb_pcg* s, int l, double out[2]);  /* lmin, lmax of level l */
void sb_pcg_mg_poly_coeffs(const sb_pcg* s, int l, double* out);      /* level l's c1, then a_j, b_j: 2 (its steps) - 1 doubles */
/* test entries, blocking, on scratch vectors; the probe is refused between sb_pcg_start and sb_pcg_finish.  probe: the transfers
 * of level l alone (l + 1 < levels): rc_out = omega_l P_l^T (r - w) and z_out = z + P_l zc.  r, w, z, z_out: n_l doubles in level
 * l's original row order; zc, rc_out: n_{l+1} doubles in level l + 1's.  first: step 1 of the post-smoothing on device vectors of
 * n doubles (16-byte aligned): d = ((r - w) * dinv) * c1, z = z + d and, with last, the ceil(n/256) level-1 values of r.z */
void sb_pcg_mg_poly_probe(sb_pcg* s, int l, const double* r_host, const double* w_host, const double* z_host, const double* zc_host,
    double* rc_out, double* z_out);
void sb_pcg_mg_poly_first_native(uint32_t n, int last, double c1, const double* r_dev, const double* w_dev, const double* dinv_dev,
    double* d_dev, double* z_dev, double* l1_rz_dev);
void sb_pcg_mg_poly_first_launch(uint32_t n, uint32_t out[3]);

/* ---- Galerkin coarse operators formed on the device ------------------------------------------------------- */
/* A_c = P^T A P for a square double-precision one-rank matrix A (n x n, any format, any permutation), read in place from its
 * upload, and a prolongation P (n x nCoarse) as a CSR triple in original numbering on both sides, as sb_pcg_create_mg_p takes it.
 * Set-up work in two row-wise products, T = A P and A_c = P^T T, every operation rounded on its own:
 *   T[i, J]   = the sum, from +0.0, of a_e * p_q over the entries e of row i of A in the order the device matrix stores the row
 *               (the order the SpMV sums it) whose stored value does not compare equal to 0.0 (Sell padding, explicit zeros) and,
 *               inside each, over the entries q of row col_e of P in storage order whose weight is not 0.0 and whose column is
 *               J; T has the entry where at least one such term exists, and nothing is dropped from it;
 *   A_c[I, J] = the sum, from +0.0, of w * T[i, J] over the entries (i, w) of row I of P^T with w != 0.0 in ascending original
 *               fine row i (equal rows: storage order) for which T[i, J] exists; an entry whose sum compares equal to 0.0 is
 *               dropped, NaN is kept.
 * The result is in the coarse level's original numbering on both sides, columns ascending, row pointers 64-bit, and the same
 * bits for A in CRS and in every Sell-C-sigma; it lives on the host.  Ends the process with a message for a single-precision
 * matrix, nr != nc (halo columns, several ranks), a P that sb_pcg_create_mg_p would refuse, intermediate storage beyond
 * sb_mem_free_bytes(), and a row of T or of P^T T with more than 1024 distinct columns (naming stage, row and the count reached:
 * never truncated). */
typedef struct sb_csr sb_csr;
sb_csr* sb_matrix_galerkin(const sb_matrix* A, uint32_t nCoarse, const uint64_t* p_ptr, const uint32_t* p_col, const double* p_val);
uint32_t sb_csr_rows(const sb_csr* c);
uint64_t sb_csr_nnz(const sb_csr* c);
void sb_csr_copy(const sb_csr* c, uint64_t* ptr, uint32_t* col, double* val); /* rows + 1, nnz, nnz entries */
/* device ms of stage 1, of stage 2 (both launches each); entries of T; entries dropped as 0.0; the largest number of distinct
 * columns of a row of T, of a row of P^T T before the drop */
void sb_csr_stats(const sb_csr* c, double out[6]);
void sb_csr_free(sb_csr* c);

/* ---- smoothed-aggregation prolongation from the matrix alone ---------------------------------------------- */
/* A prolongation for sb_pcg_create_mg_poly and sb_matrix_galerkin made on the device from a square double-precision one-rank
 * matrix in any format or permutation, read in place (no download), everything stated in ORIGINAL numbering, every
 * floating-point operation rounded on its own.  d_i is sb_matrix_diagonal's.
 *   Strong entries: a stored entry (i, j, a) with j != i, a not comparing equal to 0.0 and a*a > (theta*theta) * (fabs(d_i) *
 *     fabs(d_j)) -- no square root, a comparison with NaN is false, theta = 0 keeps every non-zero off-diagonal entry.  The graph
 *     is the directed one as stored.  A row without a strong entry is isolated: never a root, joins nothing, agg = -1.
 *   Keys, uint32 arithmetic: h = fmix32((i + 1) * 0x9E3779B1), fmix32 murmur3's (h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13;
 *     h *= 0xC2B2AE35; h ^= h >> 16); key_i = (uint64(h >> 2) << 32) | i with the state in bits 62-63: in 2, undecided 1; an out
 *     or isolated row's whole key is 0.
 *   Rounds, synchronous: m1_i = max(key_i, key_j over the strong j of row i); m2_i = max(m1_i, m1_j over the same j); an
 *     undecided row with m2_i == key_i becomes in, one whose m2_i carries the state in becomes out (the states of the round's
 *     start); until no row is undecided.  *rounds counts them up to the last one that decided a row.
 *   Aggregates: the in rows are the roots, numbered in ascending row.  Pass 1: a row that is no root and has roots among its strong
 *     entries joins the one with the largest row.  Pass 2: any other row that is not isolated joins the largest aggregate number
 *     among the pass-1 aggregates of its strong entries.
 * sb_matrix_aggregate: agg_out (nr int32, or NULL), *n_agg, *rounds; returns 0.
 * sb_matrix_sa_prolongation: T[i, agg_i] = 1.0; W = A T by sb_matrix_galerkin's first product, unchanged; P has W's pattern
 * (columns ascending, nothing dropped) and P[i, J] = t - (W[i, J] * dinv_i) * s with t = 1.0 for J == agg_i and +0.0 otherwise,
 * dinv_i = 1.0 / d_i, s = omega_s / lmax in host doubles; lmax <= 0.0: the row-sum bound of sb_pcg_create_poly.  omega_s == 0.0
 * gives T itself.  The result is read with sb_csr_copy; sb_csr_stats gives {aggregation ms, A T ms, smoothing ms, rounds, strong
 * entries, the longest row of P}.
 * Both end the process with a message, before any launch, for a single-precision matrix, nr != nc, a theta that is negative or
 * not finite, and storage beyond sb_mem_free_bytes(); behind the diagonal's launch for a diagonal entry that is zero or not
 * finite.  sb_matrix_sa_prolongation also refuses an omega_s that is negative or not finite, an lmax that is not finite, a matrix
 * without a root (every row isolated) and what the first product refuses (a row of W above 1024 columns: never truncated). */
int sb_matrix_aggregate(const sb_matrix* A, double theta, int32_t* agg_out, uint32_t* n_agg, uint32_t* rounds);
sb_csr* sb_matrix_sa_prolongation(const sb_matrix* A, double theta, double omega_s, double lmax, uint32_t* n_agg);

/* ---- BiCGStab with a diagonal preconditioner ----------------------------------------------------------- */
/* Right-preconditioned BiCGStab for matrices that need not be symmetric: two SpMVs per body, about ten vectors whatever the
 * iteration count, no restart.  x0 = 0, rhat = b; the loop test is on sqrt(r.r) alone (no exit on ||s||); rho = 0, rhat.v = 0
 * or t.t = 0 is NOT detected: the quotients become Inf or NaN and the loop runs on to itermax, as CG's does on a matrix it
 * cannot solve.  Double precision, ONE rank, tree dot order; a halo with more than one rank, a single-precision matrix, the
 * seq order, a Jacobi row whose diagonal is zero or not finite and a caller's dinv entry that is zero or not finite are fatal
 * errors with file:line.  The SpMV is the one the matrix's kernel mode selects (sb_matrix_use_packed), without a fused dot. */
typedef struct sb_bicgstab sb_bicgstab;
/* b_host, xexact_host (or NULL) as for sb_cg_create.  precond 0: none (dinv = 1.0 everywhere, dinv_host ignored); 1: Jacobi,
 * dinv_i = 1.0 / d_i with d by sb_matrix_diagonal's rule (dinv_host ignored); 2: dinv_host, nr finite non-zero doubles (either
 * sign) in ORIGINAL row order.  halo: NULL or a one-rank plan. */
sb_bicgstab* sb_bicgstab_create(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int precond,
                                const double* dinv_host);
void sb_bicgstab_free(sb_bicgstab* s);
int sb_bicgstab_solve(sb_bicgstab* s, int itermax, double eps); /* blocking; returns k of "for (k = 1; k < itermax && normr > eps; k++)" */
/* The same in three steps: bodies enqueued past the exit are no-ops, nothing is read back between bodies; a handle can be
 * solved again. */
void sb_bicgstab_start(sb_bicgstab* s, int itermax, double eps);
void sb_bicgstab_run_iters(sb_bicgstab* s, int iters);
int sb_bicgstab_finish(sb_bicgstab* s);
/* which 0: r.r, 1: rho = rhat.r (entry 0 of both is the prologue's, then one per body); 2: rhat.v, 3: t.s, 4: t.t (one per
 * body).  Copies at most cap entries to out and returns their number. */
int sb_bicgstab_history(const sb_bicgstab* s, int which, double* out, int cap);
void sb_bicgstab_solution(const sb_bicgstab* s, double* x_host);   /* original row order */
double sb_bicgstab_check_residual(const sb_bicgstab* s);           /* max|x - xexact|, 0.0 without an exact solution */
void sb_bicgstab_dinv(const sb_bicgstab* s, double* dinv_host);    /* the diagonal in use (a plan handle: level 0's dinv), original row order */
/* 10 for every format: p update | SpMV | rhat.v | alpha | s update | SpMV | t.s, t.t | omega | x, r update | beta.  On a plan
 * handle (sb_bicgstab_create_pre) with C launches per cycle: 10 + 2 C under the sweeps, 8 + 2 C under the polynomial, whose step 1
 * on level 0 rides in the two updates */
int sb_bicgstab_launches_per_body(const sb_bicgstab* s);
/* BiCGStab preconditioned by the plan of a PCG handle: ph = V(0, p) and sh = V(0, s) are the V-cycle of M's plan --
 * the sweeps, the polynomial or a cycle of either, whatever sb_pcg_create_* made.  M is BORROWED: it must outlive the handle, it
 * must have been made over m, and it must not be between sb_pcg_start and sb_pcg_finish here or at any sb_bicgstab_start (the
 * plan's level vectors are the cycle's scratch: handles that share M, and M's own solves, take turns); each of these, and what
 * sb_bicgstab_create refuses, is a fatal error with file:line.  A diagonal M without a plan: its dinv is copied, the handle is a
 * diagonal one and does not refer to M afterwards. */
sb_bicgstab* sb_bicgstab_create_pre(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, const sb_pcg* M);
int sb_bicgstab_precond(const sb_bicgstab* s); /* 0: a diagonal; else the plan's kind as sb_pcg_precond reports it */
double sb_bicgstab_loop_ms(const sb_bicgstab* s); /* GPU milliseconds between the end of sb_bicgstab_start and sb_bicgstab_finish */
void sb_bicgstab_counters(const sb_bicgstab* s, int out[5]); /* stop, iters, n_rr (= n_rho), n_rv, n_ts (= n_tt) of the control block */
/* Test entries for the fused kernels on caller-supplied device vectors of n doubles (16-byte aligned), scalars from the host;
 * blocking.  l1 arrays: ceil(n/256) level-1 values.
 *   update_p:  p = r + beta * (p - omega * v), ph = p o dinv
 *   update_s:  s = r - alpha * v, sh = s o dinv (s_dev may be r_dev)
 *   dot2:      pair != 0: level-1 values of a.b and of a.a; pair == 0: of a.b alone (l1_aa_dev untouched)
 *   update_xr: x = (x + alpha * ph) + omega * sh, r = s - omega * t (r_dev may be s_dev), level-1 values of rhat.r and r.r
 *   reduce:    the scalar step's totals of m level-1 values each: out[0] of l1_a_dev, out[1] of l1_b_dev */
void sb_bicgstab_update_p_native(uint32_t n, double beta, double omega, const double* r_dev, double* p_dev, const double* v_dev,
                                 const double* dinv_dev, double* ph_dev);
void sb_bicgstab_update_s_native(uint32_t n, double alpha, const double* r_dev, const double* v_dev, const double* dinv_dev,
                                 double* s_dev, double* sh_dev);
/* the two updates of a plan handle.  cheb 0: p (s) alone, dinv_dev, d_dev, ph_dev (sh_dev) unused and may be NULL; cheb 1: also
 * d = (p o dinv) * c1 and ph = d (the s twin: of s, into sh): level 0's first Chebyshev step */
void sb_bicgstab_plan_update_p_native(uint32_t n, int cheb, double c1, double beta, double omega, const double* r_dev, double* p_dev,
                                      const double* v_dev, const double* dinv_dev, double* d_dev, double* ph_dev);
void sb_bicgstab_plan_update_s_native(uint32_t n, int cheb, double c1, double alpha, const double* r_dev, const double* v_dev,
                                      const double* dinv_dev, double* s_dev, double* d_dev, double* sh_dev);
void sb_bicgstab_dot2_native(uint32_t n, int pair, const double* a_dev, const double* b_dev, double* l1_ab_dev, double* l1_aa_dev);
void sb_bicgstab_update_xr_native(uint32_t n, double alpha, double omega, double* x_dev, const double* ph_dev, const double* sh_dev,
                                  const double* s_dev, const double* t_dev, const double* rhat_dev, double* r_dev,
                                  double* l1_rho_dev, double* l1_rr_dev);
void sb_bicgstab_reduce_native(uint32_t m, const double* l1_a_dev, const double* l1_b_dev, double out[2]);
/* the launch of the four streaming kernels over n rows: {workgroups, threads per workgroup, compute units of the device}; a
 * wave owns whole 256-row groups and strides over them by the number of waves in the grid */
void sb_bicgstab_launch(uint32_t n, uint32_t out[3]);

/* ---- right-preconditioned GMRES(m) ------------------------------------------------------------------------ */
/* GMRES(m) on A M^-1 by a change of variable: the loop of sb_gmres_create runs unchanged on u, with w = A (M^-1 V[j]) in the
 * step and r = b - A xs, xs = M^-1 u, in the prologue and at every cycle close; sb_gmres_solution and sb_gmres_check_residual
 * give xs (the xs of the last close; 0 when no step was taken).  rr_hist is the explicit r.r of b - A xs.  M^-1 is the
 * preconditioner of the PCG handle M: its plan's V(0, .) -- the sweeps, the polynomial or a cycle of either, bit for bit
 * what sb_pcg_apply_precond gives -- or, for a handle without a plan, its diagonal.  A cycle of j steps costs j + 1 applies.
 * M is BORROWED, by sb_bicgstab_create_pre's rule: it must outlive the handle, it must have been made over m, and it must not
 * be between sb_pcg_start and sb_pcg_finish here or at any sb_gmres_start (the plan's level vectors are the cycle's scratch:
 * handles that share M -- GMRES and BiCGStab alike -- and M's own solves take turns); each of these, and what sb_gmres_create
 * refuses, is a fatal error with file:line.  A diagonal M without a plan: its dinv is copied (entries of either sign) and the
 * handle does not refer to M afterwards.  Tree dot order only.
 * sb_gmres_set_fused(s, 1) (default): the kernel that makes V[0], V[j+1] or x also writes the diagonal's product or level 0's
 * first Chebyshev step; 0: the op list, with M^-1 made wholly by the plan's own apply.  Same bits in both.
 * sb_gmres_launches_per_step: 7 + A, + 1 at j = 0, + 5 + A at j = restart - 1, with A the launches of an apply beyond what
 * rides: the cycle's under the sweeps, one fewer under the polynomial, 0 for a diagonal.  Handles that share M take turns
 * between sb_gmres_run_steps calls as well as between solves: under the polynomial the first step of a call that resumes inside
 * a cycle (j > 0) makes level 0's first step again from V[j] (one launch more than the count, the same bits), because the plan's
 * vectors may have served another handle since the step that made V[j]. */
sb_gmres* sb_gmres_create_pre(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int restart,
                              const sb_pcg* M);
/* the caller's diagonal in M^-1's place: dinv_host holds nr finite NON-ZERO doubles of either sign in original row order (a
 * PCG handle takes positive entries only); everything else as sb_gmres_create_pre with a plan-less handle */
sb_gmres* sb_gmres_create_dinv(const sb_matrix* m, sb_halo* halo, const double* b_host, const double* xexact_host, int restart,
                               const double* dinv_host);
int sb_gmres_precond(const sb_gmres* s); /* -1: none (sb_gmres_create); 0: a diagonal; else the plan's kind as sb_pcg_precond reports it */
void sb_gmres_dinv(const sb_gmres* s, double* dinv_host); /* the diagonal in use (a plan: level 0's dinv), original row order */
/* Test entries for the three riding kernels on caller-supplied device vectors (16-byte aligned); blocking.  mode -1: the
 * unfused twin (dinv_dev, d_dev, z_dev unused); 0: z = out o dinv; 1: d = z = (out o dinv) * c1.
 * scale: out = a / *scalar_dev, *g0_dev = *scalar_dev.  multiupdate: w += c[i] * V[i], ascending i, as sb_multiaxpy_sub lays V
 * out.  step: the step-and-normalise kernel at cycle position j on a throw-away state whose earlier rotations are zero:
 * hcol_host the j + 1 entries of H's column, gj = g[j], l1_dev the (n + 255) / 256 level-1 values of w . w, vnext = w / hn;
 * out_host: H's column (j + 1), cs[j], sn[j], g[j], g[j+1], the estimate, hn. */
void sb_gmres_pre_scale_native(uint32_t n, int mode, double c1, const double* a_dev, const double* scalar_dev, double* out_dev,
                               double* g0_dev, const double* dinv_dev, double* d_dev, double* z_dev);
void sb_gmres_pre_multiupdate_native(uint32_t n, int mode, double c1, int nvec, const double* V_dev, size_t ldv, const double* c_dev,
                                     double* w_dev, const double* dinv_dev, double* d_dev, double* z_dev);
void sb_gmres_pre_step_native(uint32_t n, int mode, double c1, int j, const double* hcol_host, double gj, const double* l1_dev,
                              const double* w_dev, double* vnext_dev, const double* dinv_dev, double* d_dev, double* z_dev,
                              double* out_host);

/* debug/measurement: raw streaming-read rate of the device in GB/s (DESIGN.md uses it
 * as the measured ceiling next to the 8 TB/s spec) */
double sb_debug_stream_read_gbs(size_t bytes, int reps);

const char* sb_version(void);
int sb_lab_build(void); /* always 0: there is one build (the lab build was removed) */

#ifdef __cplusplus
}
#endif
#endif /* SBHIP_H */
