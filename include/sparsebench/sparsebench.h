/* sparsebench.h -- the reference-shaped C API of the hot path, backed by the HIP layer.
 *
 * SparseBench picks its matrix format at compile time (-DCRS | -DSCS) and links
 * exactly one matrix-<FMT>.o (reference Makefile:20,32-34; src/matrix.h:14-22):
 * that link-time slot is its plugin boundary.  This header declares the same
 * symbols with the same signatures, so a driver written against the reference's
 * solver.h / matrix.h / comm.h compiles against it unchanged and links
 * libsparsebench_<fmt>.so instead of the reference objects.
 *
 * Differences a caller can observe, all additive:
 *   - Matrix gains two trailing members (`dev`, `rowNnz`) filled by convertMatrix;
 *   - Comm always carries the halo-plan members (the reference hides them behind
 *     _MPI) plus a trailing device handle;
 *   - SCS: the caller's C and sigma are honoured (the reference overwrites them
 *     with 1, src/matrix-SCS.c:42-43) and nc keeps the external columns (:38).
 *
 * Citations are paths in the reference tree.
 */
#ifndef SPARSEBENCH_H
#define SPARSEBENCH_H
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- scalar types: src/util.h:35-53 (defaults of config.mk:7-8) --------------- */
/* -DPRECISION=1 is the reference's FLOAT_TYPE=SP build (config.mk:7, 24-28): CG_FLOAT is float, the libraries are the _sp
 * ones (libsparsebench_host_sp.so, libsparsebench_<fmt>_sp.so) and every call into the HIP layer goes to its _f32 entry point
 * (SBH_FP).  Without it (or with -DPRECISION=2): double, as before. */
#if PRECISION == 1
#ifndef CG_FLOAT
#define CG_FLOAT float
#endif
#define PRECISION_STRING "single"
#define SBH_FP(name) name##_f32
#else
#ifndef CG_FLOAT
#define CG_FLOAT double
#endif
#define PRECISION_STRING "double"
#define SBH_FP(name) name
#endif
#ifndef CG_UINT
#define CG_UINT unsigned int
#endif
#define UINT_STRING      "unsigned int"
#ifndef ARRAY_ALIGNMENT
#define ARRAY_ALIGNMENT 64 /* config.mk:11 */
#endif
#define HLINE "----------------------------------------------------------------------\n"
/* src/util.h:13-33 */
#ifndef MIN
#define MIN(x, y) ((x) < (y) ? (x) : (y))
#endif
#ifndef MAX
#define MAX(x, y) ((x) > (y) ? (x) : (y))
#endif
#ifndef ABS
#define ABS(a) ((a) >= 0 ? (a) : -(a))
#endif
#ifndef IS_EQUAL
#define IS_EQUAL(a, b) (strcmp((a), (b)) == 0)
#endif
#ifndef MAXLINE
#define MAXLINE 4096
#endif
/* src/util.h:55, src/util.c:11-32: "<name up to its last dot><newEnding>", malloc'ed */
char* changeFileEnding(char* filename, char* newEnding);
#define MAX_EXTERNAL 6000000 /* src/comm.h:16 -- kept for source compatibility only */

/* ---- run-time parameters: src/parameter.h:9-18 ---------------------------------- */
typedef struct {
  char* filename;
  int nx, ny, nz;
  int itermax;
  double eps;
} Parameter;

void initParameter(Parameter*);
void readParameter(Parameter*, const char*);
void printParameter(Parameter*);

/* ---- general matrix + Matrix Market staging: src/matrix.h:24-49 ----------------- */
typedef struct {
  CG_UINT col;
  CG_FLOAT val;
} Entry;

typedef struct {
  CG_UINT nr, nc, nnz;
  CG_UINT totalNr, totalNnz;
  CG_UINT startRow, stopRow;
  CG_UINT* rowPtr;
  Entry* entries;
} GMatrix;

typedef struct {
  int row;
  int col;
  double val;
} MMEntry;

typedef struct {
  size_t count;
  int nr, nnz;
  int totalNr, totalNnz;
  int startRow, stopRow;
  MMEntry* entries;
} MMMatrix;

/* ---- format-specific matrices ----------------------------------------------------- */
/* src/CRSMatrix.h:9-16 + trailing device members */
typedef struct {
  CG_UINT nr, nc, nnz;
  CG_UINT totalNr, totalNnz;
  CG_UINT startRow, stopRow;
  CG_UINT* rowPtr;
  CG_UINT* colInd;
  CG_FLOAT* val;
  void* dev;       /* sb_matrix* in HBM (include/sbhip.h) */
  CG_UINT* rowNnz; /* nonzeros per row, for initVectors (src/CGSolver.c:27) */
} CRSMatrix;

/* src/SCSMatrix.h:13-27 + trailing device members */
typedef struct {
  CG_UINT nr, nc, nnz;
  CG_UINT totalNr, totalNnz;
  CG_UINT startRow, stopRow;
  CG_UINT* colInd;
  CG_FLOAT* val;
  CG_UINT C, sigma;
  CG_UINT nrPadded, nChunks;
  CG_UINT nElems;
  CG_UINT* chunkPtr;
  CG_UINT* chunkLens;
  CG_UINT* oldToNewPerm;
  CG_UINT* newToOldPerm;
  void* dev;
  CG_UINT* rowNnz;
} SCSMatrix;

typedef struct { /* src/SCSMatrix.h:29-32 */
  int index;
  int count;
} SellCSigmaPair;

#if defined(CRS)
typedef CRSMatrix Matrix;
#define FMT "CRS"
#elif defined(SCS)
typedef SCSMatrix Matrix;
#define FMT "SCS"
#endif

/* ---- communication: src/comm.h:25-46 ------------------------------------------------ */
enum op { MAX = 0, SUM };

typedef struct {
  int rank;
  int size;
  FILE* logFile;
  int externalCount;
  int totalSendCount;
  int* elementsToSend;
  int indegree;
  int outdegree;
  int* sources;
  int* recvCounts;
  int* rdispls;
  int* destinations;
  int* sendCounts;
  int* sdispls;
  CG_FLOAT* sendBuffer; /* unused: packing happens in HBM */
  void* dev;            /* sb_halo* */
  CG_UINT* externalGlobal; /* global id of local column nr+i */
} Comm;

/* How ranks talk during SETUP (the reference uses MPI there: Allgather :496,
 * Send/Irecv :134-161).  The launcher provides it: MPI, RCCL (sbh_exchange_rccl),
 * torch.distributed, or nothing for one rank. */
typedef struct {
  void* ctx;
  /* every rank contributes n ints; all receives size*n ints in rank order */
  void (*allgather_ints)(void* ctx, const int* mine, int n, int* all);
  /* rank r gets sendbuf[sdispls[r] .. +sendcounts[r]); counts are already known on
   * both sides */
  void (*alltoallv_ints)(void* ctx, const int* sendbuf, const int* sendcounts,
                         const int* sdispls, int* recvbuf, const int* recvcounts,
                         const int* rdispls);
} sbh_exchange;
void commSetExchange(const sbh_exchange* x); /* NULL: single rank */
const sbh_exchange* sbh_exchange_rccl(void); /* setup exchange over the RCCL communicator */

void commInit(Comm* c, int argc, char** argv);
void commFinalize(Comm* c);
void commDistributeMatrix(Comm* c, MMMatrix* m, MMMatrix* mLocal);
void commPartition(Comm* c, GMatrix* m);
void commPrintConfig(Comm* c, CG_UINT nr, CG_UINT nnz, CG_UINT startRow, CG_UINT stopRow);
/* diagnostics of the VERBOSE build, src/comm.h:54-56 (write to c->logFile when it is open) */
void commGMatrixDump(Comm* c, GMatrix* m);
void commVectorDump(Comm* c, CG_FLOAT* v, CG_UINT size, char* name); /* v: host or device */
void commExchange(Comm* c, CG_UINT numRows, CG_FLOAT* x); /* x: DEVICE vector of nc entries */
void commReduction(CG_FLOAT* v, int op);                   /* v: host or device scalar */
void commPrintBanner(Comm* c);
void commAbort(Comm* c, char* msg);
static inline int commIsMaster(Comm* c) { return c->rank == 0; }
void commBarrier(void);

/* ---- setup: src/matrix.h:51-57 ----------------------------------------------------- */
void MMMatrixRead(MMMatrix* m, char* filename);
void matrixConvertfromMM(MMMatrix* mm, GMatrix* m);
void matrixGenerate(GMatrix* m, Parameter* p, int rank, int size, bool use_7pt_stencil);
/* "irregular": deterministic irregular SPD FE-like matrix of 3*nx*ny*nz rows, the committed stand-in for
 * SuiteSparse Flan_1565 (BASELINE configs[4]; host/sbh_irregular.c).  Enters like a .mtx file: global
 * column ids, rows split over ranks by the file rule (src/comm.c:35-38), b = 1. */
void sbh_matrix_generate_irregular(GMatrix* m, Parameter* p, int rank, int size);
/* binary matrix files, src/matrixBinfile.h:21-22 (same bytes; plain POSIX I/O instead of MPI-IO;
 * SB_BMX_FP64=1 writes the fp64 extension, the reader accepts both) */
typedef struct { /* src/matrixBinfile.h:10-13: one stored nonzero of a .bmx file */
  unsigned int col;
  float val;
} FEntry;
void matrixBinWrite(GMatrix* m, Comm* c, char* filename);
void matrixBinRead(GMatrix* m, Comm* c, char* filename);
/* the driver's matrix set-up, src/main.c:54-84 (generate | generate7P | .mtx | .bmx), and its
 * `-c file.mtx` conversion, src/main.c:41-52 */
void sbh_init_matrix(Comm* c, Parameter* p, GMatrix* m);
/* commDistributeMatrix for a driver in which EVERY rank has read the file: keeps this rank's rows in place */
void sbh_distribute_local(Comm* c, MMMatrix* m, MMMatrix* mLocal);
void sbh_write_bin_matrix(Comm* c, char* mtxFilename);
/* src/allocate.h:9 -- the allocation hook.  With a device up, requests >= 64 KiB come back as memory that lives in HBM, that
 * host loops can store to and that spMVM / waxpby / ddot use in place (src/main.c:205-215 then times the kernel, not staging);
 * see host/sbh_base.c.  sbh_allocate_kind(): what the last request got -- 0 plain host, 1 device-resident and host-visible,
 * 2 pinned host.  sbh_alloc_host(): always plain host memory (what the library's own host-side arrays use).
 * spMVM and waxpby on a kind-1 vector are stream-ordered, NOT synchronous as the reference's are: call sbh_profile_sync()
 * before the host reads their output or refills one of their inputs (ddot returns its value and has waited).  Host reads cross
 * the PCIe BAR uncached: slow.  Memory from allocate() is released with sbh_allocate_free(), never with free(): kind 1 and 2
 * are not libc's. */
void* allocate(size_t alignment, size_t bytesize);
void* sbh_alloc_host(size_t alignment, size_t bytesize);
int sbh_allocate_kind(void);
void sbh_allocate_free(void* p);
size_t sbh_device_free_bytes(void); /* free device memory, bytes */
double getTimeStamp(void);                          /* src/timing.h:8 */
double getTimeResolution(void);                     /* src/timing.h:9 */

/* runtime-format entry points (what the drop-in symbols below forward to) */
void sbh_convert_crs(CRSMatrix* m, GMatrix* im);
void sbh_convert_scs(SCSMatrix* m, GMatrix* im); /* honours m->C, m->sigma set by the caller */
void sbh_spmv(void* dev_matrix, CG_UINT nr, CG_UINT nc, const CG_FLOAT* x, CG_FLOAT* y);
int sbh_solve_cg(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr,
                 const CG_UINT* rowNnz);
/* restarted GMRES(restart) on the same matrix (sb_gmres_*, sbhip.h): prints what solveCG prints; double precision, one rank */
int sbh_solve_gmres(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr,
                    const CG_UINT* rowNnz, int restart);
/* batched CG (sb_cgb_*, sbhip.h): nrhs independent CG solves on one pass over the matrix per body; startRow: the global index
 * of local row 0 (the right-hand sides of columns >= 1 are a function of the global row index); double precision, one rank */
int sbh_solve_cg_batch(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, CG_UINT startRow,
                       int nrhs);
/* CG with the Jacobi preconditioner dinv = 1 / diag(A) (sb_pcg_*, sbhip.h): prints what solveCG prints; double precision, one rank */
int sbh_solve_pcg(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz);
/* the same with symmetric Gauss-Seidel by multicolouring in the diagonal's place (sb_pcg_create_sgs, sbhip.h); first prints
 * "Preconditioner: SGS ..., nC = <colours>" */
int sbh_solve_pcg_sgs(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz);
/* the same with a multigrid V-cycle around that smoother (sb_pcg_create_mg, sbhip.h) on the geometric hierarchy of
 * a generated matrix: level l + 1 is the same generator on half the grid in every direction, in the fine matrix's format (fmt: 0
 * CRS, 1 Sell-C-sigma with C and sigma).  levels: L, or 0 for the deepest L <= 4 the grid allows.  First prints "Preconditioner:
 * MG ..., levels = L, nC = <colours of level 0>".  A matrix from a file, or a grid that does not allow L levels, ends the
 * process with a message. */
int sbh_solve_pcg_mg(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int fmt, CG_UINT C,
                     CG_UINT sigma, int levels);
/* sbh_solve_pcg_mg with full-weighting transfers in the injection's place (sb_pcg_create_mg_p, sbhip.h): the
 * trilinear prolongation of sbh_mg_trilinear and omega = 0.5 between every two levels; the same depth rules and refusals.  First
 * prints "Preconditioner: MG (V-cycle, full-weighting transfers, multicolour SGS smoother), levels = L, nC = <colours>" */
int sbh_solve_pcg_mgfw(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int fmt, CG_UINT C,
                       CG_UINT sigma, int levels);
/* sbh_solve_pcg_mgfw with the Chebyshev polynomial as the smoother of every level (sb_pcg_create_mg_poly, sbhip.h):
 * the regenerated hierarchy, the trilinear prolongation with omega = 0.25, steps per smoothing (1 .. 16; 0: the default 2) on
 * [lmax_l / 4, lmax_l] per level; the same depth rules and refusals.  First prints "Preconditioner: MG (V-cycle, full-weighting
 * transfers, Chebyshev polynomial smoother), levels = L, steps = <steps>, lambda in [<lmin>, <lmax> of level 0]" */
int sbh_solve_pcg_mgpoly(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int fmt, CG_UINT C,
                         CG_UINT sigma, int levels, int steps);
/* sbh_solve_pcg_mgpoly on Galerkin coarse operators in the regenerated ones' place: A_{l+1} = P_l^T A_l P_l formed
 * on the device (sbh_mg_hierarchy_build_galerkin), omega = 1.0; the same depth rules, refusals and default steps.  The
 * preconditioner line says "Galerkin coarse operators"; a second line gives the products' device milliseconds per level */
int sbh_solve_pcg_mgpoly_galerkin(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int fmt,
                                  CG_UINT C, CG_UINT sigma, int levels, int steps);
/* sbh_solve_pcg with a Chebyshev polynomial in D^-1 A in the diagonal's place (sb_pcg_create_poly, sbhip.h): steps
 * terms (1 .. 16; 0: the default 3) on [lmax / 16, lmax], lmax by the row-sum bound of D^-1/2 A D^-1/2.  First prints
 * "Preconditioner: Chebyshev polynomial, steps = <steps>, lambda in [<lmin>, <lmax>]" */
int sbh_solve_pcg_poly(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int steps);
/* the geometric hierarchy's rule: L levels need every dimension divisible by 2^(L-1) and every coarse dimension >= 2.  want: L, or
 * 0 for the deepest L <= 4.  Returns L, or 0 with the reason in why (cap bytes) */
int sbh_mg_levels(int nx, int ny, int nz, int want, char* why, size_t cap);
/* the injection map of an nx x ny x nz grid (all even): coarse point (x, y, z) of the (nx/2) x (ny/2) x (nz/2) grid is fine
 * point (2x, 2y, 2z), both in the generator's lexicographic numbering (x fastest); f2c holds (nx/2)(ny/2)(nz/2) entries */
void sbh_mg_f2c(int nx, int ny, int nz, CG_UINT* f2c);
/* the trilinear prolongation of an nx x ny x nz grid (all even) from the grid of half the size in every direction, as CSR over the
 * nx ny nz fine points, both sides in the generator's numbering (x fastest): per dimension an even index i takes coarse i / 2 with
 * weight 1, an odd one (i - 1) / 2 and (i + 1) / 2 with 1/2 each, the second dropped (not renormalised) where it would be the
 * coarse dimension itself; a row's weights are the products 1, 1/2, 1/4, 1/8, its entries in ascending coarse number.  ptr holds
 * nx ny nz + 1 entries; col and val room for 8 per row.  With it goes omega = 0.5 */
void sbh_mg_trilinear(int nx, int ny, int nz, uint64_t* ptr, CG_UINT* col, double* val);
/* the L - 1 coarse levels of param's grid in the fine matrix's format, generated, converted and uploaded as the driver does the
 * fine one: mats[l - 1] (an sb_matrix*) and maps[l - 1] are level l's device matrix and the injection map into it, l = 1 .. L - 1.
 * Returns what sbh_mg_hierarchy_free releases (after the solver handle that uses the levels) */
void* sbh_mg_hierarchy_build(const Parameter* param, int fmt, CG_UINT C, CG_UINT sigma, int L, const void** mats, const CG_UINT** maps);
void sbh_mg_hierarchy_free(void* hierarchy, int fmt, int L);
/* the Galerkin mode of the builder: level l + 1 is P_l^T A_l P_l with the trilinear P_l of level l's grid, formed on
 * the device from level l's UPLOADED matrix (sb_matrix_galerkin, sbhip.h; fine_dev is level 0's), put into a GMatrix and taken
 * through the same commPartition -> convert (the fine level's C and sigma) -> upload as a regenerated level.  mats[l - 1] is level
 * l's device matrix, p_ptr / p_col / p_val[l - 1] the prolongation INTO level l - 1 from it (owned by the hierarchy: they live
 * until sbh_mg_hierarchy_free), stage_ms[2 (l - 1)] and [2 (l - 1) + 1] the device milliseconds of the product's two stages
 * (NULL: not wanted).  omega = 1.0 goes with it.  Double precision, one rank. */
void* sbh_mg_hierarchy_build_galerkin(const Parameter* param, const void* fine_dev, int fmt, CG_UINT C, CG_UINT sigma, int L,
    const void** mats, const uint64_t** p_ptr, const CG_UINT** p_col, const double** p_val, double* stage_ms);
/* the aggregation mode of the builder, for ANY square one-rank double-precision matrix: no grid.  Level l + 1 is
 * P_l^T A_l P_l with P_l = sb_matrix_sa_prolongation(level l's uploaded matrix, theta, omega_s, its own row-sum bound), both formed
 * on the device, then GMatrix -> commPartition -> convert -> upload as sbh_mg_hierarchy_build_galerkin does.  Stops at maxL levels
 * or at the first level of at most SBH_MG_SA_COARSEST rows; *L_out is the depth reached (free with it).  mats, p_ptr, p_col, p_val
 * as there (room for maxL entries each); rows[l] level l's rows (maxL entries), rounds[l] the rounds of level l's aggregation,
 * ms[3 l], [3 l + 1], [3 l + 2] the device milliseconds of level l's aggregation, of A T with the smoothing, and of the Galerkin
 * product (NULL: not wanted).  A level that coarsens by less than 2 ends the process with a message naming it; a level without a
 * root is the library's refusal.  omega = 1.0 goes with it. */
#define SBH_MG_SA_COARSEST 64
#define SBH_MG_SA_DEPTH 4
void* sbh_mg_hierarchy_build_sa(const void* fine_dev, CG_UINT fine_nr, int fmt, CG_UINT C, CG_UINT sigma, int maxL, double theta,
    double omega_s, int* L_out, const void** mats, const uint64_t** p_ptr, const CG_UINT** p_col, const double** p_val, CG_UINT* rows,
    CG_UINT* rounds, double* ms);
/* sbh_solve_pcg_mgpoly on that hierarchy (theta = 0, omega_s = 4/3; levels 0: up to SBH_MG_SA_DEPTH), on generated matrices and
 * files alike.  The preconditioner line says "smoothed-aggregation coarsening"; a second line gives every level's rows and the
 * rounds of every aggregation, a third the set-up's device milliseconds per level */
int sbh_solve_pcg_mgpoly_sa(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int fmt, CG_UINT C,
                            CG_UINT sigma, int levels, int steps);
/* a one-rank GMatrix of n rows from CSR in memory (64-bit row pointers): a row's entries end up in ascending column, storage order
 * kept among equal columns -- what reading the same entries from a .mtx file gives */
void sbh_gmatrix_from_csr(GMatrix* m, CG_UINT n, const uint64_t* ptr, const CG_UINT* col, const double* val);
/* BiCGStab with the Jacobi right preconditioner (sb_bicgstab_*, sbhip.h) for matrices that need not be symmetric: prints what
 * solveCG prints; double precision, one rank */
int sbh_solve_bicgstab(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz);
/* BiCGStab with a preconditioner plan of PCG's in the diagonal's place (sb_bicgstab_create_pre, sbhip.h): precond 1
 * sgs, 2 mg, 3 mgfw, 4 poly, 5 mgpoly (galerkin 1: on Galerkin coarse operators formed on the device; 2: on the aggregation hierarchy); levels, steps 0: the
 * defaults; fmt, C, sigma as sbh_solve_pcg_mg takes them (used by the V-cycles only).  The PCG handle is built as the
 * sbh_solve_pcg_* entries build theirs and the same "Preconditioner: ..." line is printed first; the same refusals.  Double
 * precision, one rank */
int sbh_solve_bicgstab_precond(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int fmt, CG_UINT C,
                               CG_UINT sigma, int precond, int levels, int steps, int galerkin);

/* ---- the hot path: src/solver.h:11-25, src/matrix.h:57 -------------------------------- */
/* GMRES(restart) right-preconditioned by one of PCG's preconditioners (sb_gmres_create_pre, sbhip.h): GMRES on
 * A M^-1, the solution x = M^-1 u.  precond 0 jacobi, 1 sgs, 2 mg, 3 mgfw, 4 poly, 5 mgpoly (galerkin 1: on Galerkin coarse
 * operators formed on the device; 2: on the aggregation hierarchy); levels, steps 0: the defaults; fmt, C, sigma as
 * sbh_solve_pcg_mg takes them (used by the V-cycles only).  The PCG handle is built as the sbh_solve_pcg_* entries build theirs
 * and freed after the solver; the same "Preconditioner: ..." line is printed first; the same refusals.  Double precision, one rank */
int sbh_solve_gmres_precond(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int fmt, CG_UINT C,
    CG_UINT sigma, int restart, int precond, int levels, int steps, int galerkin);

/* ---- one spec and one entry behind the add-on solvers above, and the driver's options ------------------ */
/* the preconditioner kinds, with the numbers -p, -P, solveBiCGStabPrecond and solveGMRESPrecond give them; NONE: none was named */
enum { SBH_PRECOND_NONE = -1, SBH_PRECOND_JACOBI = 0, SBH_PRECOND_SGS, SBH_PRECOND_MG, SBH_PRECOND_MGFW, SBH_PRECOND_POLY, SBH_PRECOND_MGPOLY };
/* the coarse operators of SBH_PRECOND_MGPOLY: the stencil regenerated on every coarser grid, P^T A P formed on the device with
 * the trilinear P, or the smoothed-aggregation hierarchy made from the matrix alone */
enum { SBH_COARSE_REGENERATED = 0, SBH_COARSE_GALERKIN, SBH_COARSE_AGGREGATION };
enum { SBH_SOLVER_PCG = 0, SBH_SOLVER_BICGSTAB, SBH_SOLVER_GMRES };
/* a preconditioner as every entry above names it: levels (the V-cycles) and steps (poly, mgpoly) 0: the default */
typedef struct {
  int kind, levels, steps, coarse;
} sbh_precond_spec;
/* What every sbh_solve_pcg*, sbh_solve_bicgstab* and sbh_solve_gmres* entry above is a one-line call of (they remain): solver
 * SBH_SOLVER_* with the preconditioner of spec, restart for GMRES only; fmt, C, sigma as sbh_solve_pcg_mg takes them (used by
 * the V-cycles only).  spec NULL: PCG's Jacobi, and BiCGStab or GMRES alone (sbh_solve_bicgstab, sbh_solve_gmres); with a spec
 * those two borrow PCG's plan (one rank; BiCGStab's own diagonal is not a kind of its).  Prints the "Preconditioner: ..." line
 * of the kind first (PCG's Jacobi: none, the driver prints it).  Double precision */
int sbh_solve_precond(Comm* comm, Parameter* param, void* dev_matrix, CG_UINT nr, const CG_UINT* rowNnz, int fmt, CG_UINT C,
    CG_UINT sigma, int solver, int restart, const sbh_precond_spec* spec);
static inline int sbh_is_generated(const Parameter* param)
{
  return strcmp(param->filename, "generate") == 0 || strcmp(param->filename, "generate7P") == 0;
}

/* The benchmark driver's command line, parsed without a device (host/sbh_options.c): no Comm, no sb_* call, no exit, no output */
enum { SBH_BENCH_CG = 0, SBH_BENCH_SPMV, SBH_BENCH_GMRES, SBH_BENCH_PCG, SBH_BENCH_BICGSTAB };
enum { SBH_ACT_RUN = 0, SBH_ACT_HELP, SBH_ACT_CONVERT }; /* what the caller does next: set up and run, print the help, write <file> as .bmx */
typedef struct {
  int type;                 /* -t: SBH_BENCH_* */
  int restart, nrhs;        /* -r, -n */
  unsigned scsC, scsSigma;  /* -C, -s */
  int byP;                  /* the preconditioner came by -P (BiCGStab's, GMRES's), not by -p */
  sbh_precond_spec precond; /* -p or -P with -l, -d and -g or -a */
  int optind;               /* the first non-option argument (argc: none, or the parse ended inside the options) */
  int action;               /* SBH_ACT_* */
  char* convert;            /* SBH_ACT_CONVERT: -c's <file> */
  int toStdout;             /* of a refusal: its message goes to stdout (the unknown -t), not to stderr */
} sbh_options;
/* Parses argv into param and o as the driver always has, checks in the same order.  Returns 0, or 1 for a refusal with its
 * message (the newline included) in msg.  -h and -c end the parse where they stand: what came before them is applied, what
 * follows is not looked at.  Resets getopt's state, so it can be called again; param->filename may point into argv */
int sbh_parse_options(int argc, char** argv, Parameter* param, sbh_options* o, char* msg, size_t cap);
const char* sbh_help_text(void);
/* What of the parsed options runs on `size` ranks, checked without a device as well: -t cg, -t spmv, and -t pcg with the Jacobi
 * diagonal or -p poly [-d n].  Returns 0, or 1 with "<who>: runs on one rank\n" in msg for -p sgs ("SGS"), -p mg |
 * mgfw | mgpoly with or without -g and -a ("MG"), -t gmres and -t bicgstab; size < 2: 0 */
int sbh_check_ranks(const sbh_options* o, int size, char* msg, size_t cap);
#if defined(CRS) || defined(SCS)
/* the fmt, C, sigma arguments of the entries above that rebuild the matrix on coarser grids, for this build's Matrix */
#ifdef SCS
#define SBH_FMT_ARGS(m) 1, (m)->C, (m)->sigma
#else
#define SBH_FMT_ARGS(m) 0, 0, 0
#endif
void convertMatrix(Matrix* m, GMatrix* im);
int solveCG(Comm* comm, Parameter* param, Matrix* m);
/* the solver the reference's driver names and leaves empty (src/main.c:31,217-222): restarted GMRES(restart) for matrices
 * that are not symmetric positive definite; returns k as solveCG does.  The single-precision libraries export it too and
 * end the process with "GMRES: double precision only". */
int solveGMRES(Comm* comm, Parameter* param, Matrix* m, int restart);
/* nrhs (2, 4 or 8) independent CG solves on ONE stream of the matrix per loop body.  Column 0's right-hand side
 * is initVectors' b (and xexact); for c >= 1, b_c[i] = b_0[i] + c * ((g(i) mod 5) - 2) with g the global row index, without
 * an exact solution.  Prints solveCG's lines per column, each prefixed "RHS c: ", then the usual "Solution performed %d
 * iterations and took %.2fs" with the largest k_c and the residual check of column 0; returns the largest k_c.  Column c's
 * numbers are bit for bit those of solveCG on b_c alone.  One rank, tree dot order; the single-precision libraries export it
 * too and end the process with "batched CG: double precision only". */
int solveCGBatch(Comm* comm, Parameter* param, Matrix* m, int nrhs);
/* solveCG with the Jacobi preconditioner put back: z = r o (1 / diag(A)), alpha = r.z / p.Ap, beta = r.z / (r.z)_old,
 * the loop test on sqrt(r.r) as in solveCG.  Prints solveCG's lines from the recorded history and returns k as solveCG does.
 * A matrix row without a finite positive diagonal entry ends the process with a message.  Tree dot order; one rank or several
 * (the Comm's halo plan fills p's halo ahead of every SpMV, each dot is the rank's tree-order value then the pairwise
 * tree over ranks; collective like solveCG); the single-precision libraries export it too and end the process with "PCG: double
 * precision only". */
int solvePCG(Comm* comm, Parameter* param, Matrix* m);
/* solvePCG with HPCG's own preconditioner, symmetric Gauss-Seidel, applied by multicolouring: z = M^-1 r with
 * M = (D + L) D^-1 (D + U) in a greedy colour order of the rows, one launch per colour and sweep.  Prints the preconditioner and
 * its colour count, then solvePCG's lines; returns k as solveCG does.  Square matrix, one rank, tree dot order; a row without a
 * finite positive diagonal entry ends the process with a message; the single-precision libraries export it too and end the
 * process with "PCG: double precision only". */
int solvePCGSGS(Comm* comm, Parameter* param, Matrix* m);
/* solvePCG with HPCG's whole preconditioner: a geometric multigrid V-cycle with that symmetric Gauss-Seidel smoother, injection
 * and the same stencil regenerated on each coarser grid, at the deepest of up to 4 levels the grid allows.  For
 * matrices made by "generate" or "generate7P" with param's nx, ny, nz: a matrix from a file ends the process with "needs the
 * grid".  Prints the preconditioner, its levels and level 0's colour count, then solvePCG's lines; returns k as solveCG does.
 * One rank, tree dot order; the single-precision libraries export it too and end the process with "PCG: double precision only". */
int solvePCGMG(Comm* comm, Parameter* param, Matrix* m);
/* solvePCGMG with trilinear interpolation and its scaled transpose applied to the full residual between the levels:
 * the transfers with which the coarse levels count in every row order.  The same matrices, refusals, printed lines (the
 * preconditioner line says "full-weighting transfers") and return value. */
int solvePCGMGFW(Comm* comm, Parameter* param, Matrix* m);
/* solvePCG with a Chebyshev polynomial preconditioner: z = q(D^-1 A) D^-1 r, three terms of the Chebyshev recurrence
 * on [lmax / 16, lmax], each term behind the first one SpMV of the matrix's own and a streaming kernel; no colouring, no set-up
 * beyond a row-sum bound for lmax.  Prints the preconditioner, its steps and interval, then solvePCG's lines; returns k as solveCG
 * does.  Tree dot order; one rank (a square matrix) or several as solvePCG runs on them (lmax is then the MAX over ranks of the
 * bound, and z's halo is filled ahead of every step's SpMV); a row without a finite positive diagonal entry ends the process with
 * a message; the single-precision libraries export it too and end the process with "PCG: double precision only". */
int solvePCGPoly(Comm* comm, Parameter* param, Matrix* m);
/* solvePCGMGFW with that polynomial as the smoother of every level in the Gauss-Seidel sweeps' place: two steps
 * before and after on every level, omega = 0.25, every SpMV of the cycle the level's own; no colouring.  The same matrices and
 * refusals; the preconditioner line names the smoother, its steps and level 0's interval. */
int solvePCGMGPoly(Comm* comm, Parameter* param, Matrix* m);
/* solvePCGMGPoly on Galerkin coarse operators P^T A P, formed on the device from the uploaded matrices, in the regenerated
 * stencils' place; omega = 1.0.  The same matrices and refusals; the preconditioner line says "Galerkin coarse
 * operators" and a second line gives the products' device time per level. */
int solvePCGMGPolyGalerkin(Comm* comm, Parameter* param, Matrix* m);
/* solvePCGMGPoly on the smoothed-aggregation hierarchy made from the matrix alone: any square matrix, generated or
 * read from a file; theta = 0, omega_s = 4/3, up to 4 levels, omega = 1.0.  The preconditioner line says "smoothed-aggregation
 * coarsening"; two more lines give the level sizes with the rounds, and the set-up's device time per level. */
int solvePCGMGPolySA(Comm* comm, Parameter* param, Matrix* m);
/* Jacobi-preconditioned BiCGStab: the short-recurrence solver for matrices that are not symmetric; returns k as
 * solveCG does.  The single-precision libraries export it too and end the process with "BiCGStab: double precision only". */
int solveBiCGStab(Comm* comm, Parameter* param, Matrix* m);
/* solveBiCGStab with one of PCG's preconditioners in the diagonal's place: precond 1 sgs, 2 mg, 3 mgfw, 4 poly,
 * 5 mgpoly, each at its defaults and built as the solvePCG* entry of that name builds it (the V-cycles: generated matrices only).
 * Prints that entry's preconditioner line, then solveBiCGStab's lines; returns k as solveCG does.  One rank; the single-precision
 * libraries export it too and end the process with "BiCGStab: double precision only". */
int solveBiCGStabPrecond(Comm* comm, Parameter* param, Matrix* m, int precond);
/* solveGMRES right-preconditioned by one of PCG's preconditioners: precond 0 jacobi, 1 sgs, 2 mg, 3 mgfw, 4 poly,
 * 5 mgpoly, each at its defaults and built as the solvePCG* entry of that name builds it (the V-cycles: generated matrices only).
 * Prints that entry's preconditioner line, then solveGMRES's lines; returns k as solveCG does.  One rank; the single-precision
 * libraries export it too and end the process with "GMRES: double precision only". */
int solveGMRESPrecond(Comm* comm, Parameter* param, Matrix* m, int restart, int precond);
/* x (nc entries) and y (nr entries) may be device or host pointers; host pointers are
 * staged through HBM (correct, slow: use sb_malloc'ed vectors on the hot path) */
void spMVM(Matrix* m, const CG_FLOAT* restrict x, CG_FLOAT* restrict y);
void commMatrixDump(Comm* c, Matrix* m); /* src/comm.h:55 */
#endif
void waxpby(const CG_UINT n, const CG_FLOAT alpha, const CG_FLOAT* restrict x,
            const CG_FLOAT beta, const CG_FLOAT* restrict y,
            CG_FLOAT* w /* may alias x or y, as src/CGSolver.c:114,127 do (the reference's
                           definition drops `restrict` here too, src/solver.c:21) */);
void ddot(const CG_UINT n, const CG_FLOAT* restrict x, const CG_FLOAT* restrict y,
          CG_FLOAT* restrict result);

/* ---- profiler: src/profiler.h:10-30 --------------------------------------------------- */
typedef enum { WAXPBY = 0, SPMVM, DDOT, COMM, NUMREGIONS } regions;
extern double _t[NUMREGIONS];
/* The reference reads the host clock around a synchronous CPU call (src/profiler.h:18-21).  Here `call` is a stream-ordered
 * launch: the region is bracketed by two device events (sbh_region_begin / _end), nothing waits inside the caller's loop, and
 * profilerPrint() reports the accumulated DEVICE time of every tag that recorded regions (the host-side enqueue time is still
 * added to _t[tag], as the reference does, and is what the table falls back to for a tag without regions). */
#define PROFILE(tag, call)                                                     \
  ts = getTimeStamp();                                                         \
  sbh_region_begin(tag);                                                       \
  call;                                                                        \
  sbh_region_end(tag);                                                         \
  _t[tag] += (getTimeStamp() - ts);
void sbh_region_begin(int tag);
void sbh_region_end(int tag);
void sbh_profile_sync(void); /* waits for the layer's stream (callers that time with the host clock themselves) */
void profilerInit(size_t* facFlops, size_t* facWords);
void profilerPrint(Comm* c, int iterations);
void profilerFinalize(void);

#ifdef __cplusplus
}
#endif
#endif /* SPARSEBENCH_H */
