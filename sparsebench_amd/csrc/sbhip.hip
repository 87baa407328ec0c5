// sbhip.hip -- implementation of the C-ABI in include/sbhip.h.
//
// One process drives one MI355X.  All work goes to one HIP stream; the CG loop
// keeps alpha, beta, rtrans and the loop-exit flag in HBM so no host round trip
// happens between iterations.  RCCL is opened lazily (dlopen) only when a
// communicator is attached, so single-GPU runs never load it.
#include "../../include/sbhip.h"

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include <setjmp.h>
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kernels.hip.h"
#include "kernels_sp.hip.h"
#include "kernels_sp_comm.hip.h"
#include "pack.hip.h"
#include "pack_sp.hip.h"
#include "gmres.hip.h"
#include "batch.hip.h"
#include "pcg.hip.h"
#include "sgs.hip.h"
#include "bicgstab.hip.h"
#include "mg.hip.h"
#include "mg_fw.hip.h"
#include "poly.hip.h"
#include "mg_poly.hip.h"
#include "galerkin.hip.h"
#include "aggregation.hip.h"

#include <algorithm>
#include <iterator>
#include <string>
#include <unordered_map>

using namespace sbk;

#ifndef SB_FUSE_P_DEFAULT
#define SB_FUSE_P_DEFAULT true // the p update inside the SpMV (spmv_prog_fusep) wherever it applies: measured faster at every
                               // size and format (128^3 sigma 256 +5 %, sigma 1 +12 %, CRS mirror +10 %, 64^3 +20 %); SB_FUSE_P=0 /
                               // sb_cg_set_fuse_p(s, 0) keep the separate p update
#endif

#define HIP_CHECK(call)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) {                                                               \
      fprintf(stderr, "sbhip: HIP error %s at %s:%d: %s\n", hipGetErrorName(e_), __FILE__, \
          __LINE__, hipGetErrorString(e_));                                               \
      exit(EXIT_FAILURE);                                                                 \
    }                                                                                     \
  } while (0)

#define SB_FATAL(...)                                        \
  do {                                                       \
    fprintf(stderr, "sbhip: %s:%d: ", __FILE__, __LINE__);   \
    fprintf(stderr, __VA_ARGS__);                            \
    fprintf(stderr, "\n");                                   \
    exit(EXIT_FAILURE);                                      \
  } while (0)

// ---------------------------------------------------------------------------
// RCCL, bound at run time
// ---------------------------------------------------------------------------
namespace {
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
enum { ncclSuccess_ = 0 };
enum { ncclInt8_ = 0, ncclInt32_ = 2, ncclFloat32_ = 7, ncclFloat64_ = 8 }; // ncclDataType_t
enum { ncclSum_ = 0, ncclMax_ = 2 }; // ncclRedOp_t

struct Rccl {
  void* h = nullptr;
  int (*GetUniqueId)(ncclUniqueId*);
  int (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int);
  int (*CommDestroy)(ncclComm_t);
  int (*AllReduce)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t);
  int (*AllGather)(const void*, void*, size_t, int, ncclComm_t, hipStream_t);
  int (*Send)(const void*, size_t, int, int, ncclComm_t, hipStream_t);
  int (*Recv)(void*, size_t, int, int, ncclComm_t, hipStream_t);
  int (*GroupStart)();
  int (*GroupEnd)();
  const char* (*GetErrorString)(int);
  int (*CommCount)(ncclComm_t, int*);    // optional (diagnostics only)
  int (*CommUserRank)(ncclComm_t, int*); // optional
  int (*CommCuDevice)(ncclComm_t, int*); // optional
} rccl;

void rccl_open()
{
  if (rccl.h) return;
  const char* names[] = { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" };
  for (const char* n : names) {
    rccl.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (rccl.h) break;
  }
  if (!rccl.h) SB_FATAL("cannot open librccl: %s", dlerror());
#define BIND(field, sym)                                           \
  *(void**)(&rccl.field) = dlsym(rccl.h, sym);                     \
  if (!rccl.field) SB_FATAL("librccl lacks %s", sym)
  BIND(GetUniqueId, "ncclGetUniqueId");
  BIND(CommInitRank, "ncclCommInitRank");
  BIND(CommDestroy, "ncclCommDestroy");
  BIND(AllReduce, "ncclAllReduce");
  BIND(AllGather, "ncclAllGather");
  BIND(Send, "ncclSend");
  BIND(Recv, "ncclRecv");
  BIND(GroupStart, "ncclGroupStart");
  BIND(GroupEnd, "ncclGroupEnd");
  BIND(GetErrorString, "ncclGetErrorString");
#undef BIND
  *(void**)(&rccl.CommCount)    = dlsym(rccl.h, "ncclCommCount");
  *(void**)(&rccl.CommUserRank) = dlsym(rccl.h, "ncclCommUserRank");
  *(void**)(&rccl.CommCuDevice) = dlsym(rccl.h, "ncclCommCuDevice");
}
#define RCCL_CHECK(call)                                                                  \
  do {                                                                                    \
    int r_ = (call);                                                                      \
    if (r_ != ncclSuccess_)                                                               \
      SB_FATAL("RCCL error %d (%s)", r_, rccl.GetErrorString ? rccl.GetErrorString(r_) : "?"); \
  } while (0)

struct Ctx {
  bool init = false;
  int device = 0;
  hipStream_t stream = nullptr;
  hipDeviceProp_t prop;
  char name[320];
  // scratch for stand-alone ddot / permuted sb_spmv
  double* partials = nullptr;
  size_t partialsCap = 0;
  double* scalar = nullptr; // one device double
  double* ws[2] = { nullptr, nullptr };
  size_t wsCap[2] = { 0, 0 };
  // communicator: RCCL, or a caller-provided host-mediated transport (sb_comm_init_transport)
  ncclComm_t comm = nullptr;
  int rank = 0, size = 1;
  bool hasXport = false;
  sb_transport xport;
  // in-kernel all-reduce over peer-mapped memory (kernels.hip.h: p2p_allreduce_sum)
  P2PSlot* p2pBuf = nullptr;        // this rank's buffer (fine-grained device memory), P2PSlot[2][P2P_MAX]
  void* p2pPeer[P2P_MAX] = {};      // peers' buffers as opened here (IPC); [rank] = p2pBuf
  P2PView* p2pView = nullptr;       // device copy of the view
  unsigned long long p2pSeq = 0;    // exchanges issued so far (identical on every rank)
  bool p2pOn = false;
  bool pushInside = false;          // sb_comm_halo_push_inside (initialised from SB_HALO_PUSH_INSIDE at sb_init)
  bool p2pUse = true;               // sb_comm_data_plane: 0 = run on the communicator's collectives although the mappings exist
  char p2pReason[256] = "not set up (one rank, or no communicator yet)"; // why the path is on / off
  long long p2pTimeoutTicks = 30000 * P2P_TICKS_PER_MS; // waits inside CG (SB_P2P_TIMEOUT_MS)
  float* rankValsF = nullptr;       // sb_comm_reduction_f32 over RCCL: the all-gathered rank values (size floats)
} g;

inline bool multi_rank() { return g.comm != nullptr || g.hasXport; }
// the peer-mapped data plane is set up AND selected (sb_comm_data_plane)
inline bool p2p_dots() { return g.p2pOn && g.p2pUse; }
// a stop flag that is never set, for launches outside a CG loop (kernels that fetch the flag
// together with other data want a valid address)
inline const int* zero_flag() { return reinterpret_cast<const int*>(g.scalar + 4); }

void need_init()
{
  if (!g.init) SB_FATAL("sb_init() has not been called");
}

double* scratch_partials(size_t n)
{
  if (n > g.partialsCap) {
    if (g.partials) HIP_CHECK(hipFree(g.partials));
    g.partialsCap = n + n / 2 + 1024;
    HIP_CHECK(hipMalloc(&g.partials, g.partialsCap * sizeof(double)));
  }
  return g.partials;
}

double* scratch_ws(int which, size_t n)
{
  if (n > g.wsCap[which]) {
    if (g.ws[which]) HIP_CHECK(hipFree(g.ws[which]));
    g.wsCap[which] = n;
    HIP_CHECK(hipMalloc(&g.ws[which], n * sizeof(double)));
  }
  return g.ws[which];
}

inline uint32_t stream_grid(uint32_t nWork, uint32_t perBlock)
{ // memory-bound grid: enough blocks to fill 256 CUs x 8, grid-stride the rest
  uint32_t b   = (nWork + perBlock - 1) / perBlock;
  uint32_t cap = (uint32_t)g.prop.multiProcessorCount * 8u;
  if (b > cap) b = cap;
  return b ? b : 1;
}
} // namespace

struct sb_matrix {
  int fmt; // 0 CRS, 1 SCS
  uint32_t nr, nc, nnz;
  // CRS
  uint32_t *rowPtr = nullptr, *rowBlocks = nullptr;
  uint32_t nRowBlocks = 0;
  uint32_t* tileRow = nullptr; // spmv_crs_split: first row starting at or behind nonzero lb * crsT (NULL: a row is too long)
  uint32_t nCrsTiles = 0, crsT = 0;
  // SCS
  uint32_t C = 0, sigma = 0, nChunks = 0, nElems = 0, nrPadded = 0;
  uint32_t *chunkPtr = nullptr, *chunkLens = nullptr;
  uint32_t *oldToNew = nullptr, *newToOld = nullptr; // device, nr each (SCS permuted only)
  int permuted = 0;
  // both
  uint32_t* colInd = nullptr;
  double* val = nullptr;
  // placement (sb_matrix_place): the reference-layout stream inside ONE slab at chosen offsets; colInd / val then point into it
  char* slab         = nullptr;
  size_t slabBytes   = 0;
  uint32_t* colInd0  = nullptr; // the arrays as first uploaded (source of every re-placement; freed once the placement is final)
  double* val0       = nullptr;
  int placeColMB = -1, placeValMB = -1;
  std::vector<char*> oldSlabs; // sb_matrix_place_fresh: earlier slabs, kept allocated until the placement is final
  float placeUs[3] = { 0.f, 0.f, 0.f }; // the tuner's proxy-step times: first arena + hipMalloc's own placement, the pair kept, the slowest seen
  int placeTried = 0;                   // probes the tuner timed (0: it did not run)
  char* vecArena = nullptr;             // the allocation the tuner found best for the loop's vectors: the next sb_cg_create uses it
  size_t vecArenaBytes = 0;
  bool vecArenaBusy = false;
  // SCS C=64: device-private compressed mirror (pack.hip.h)
  PackMeta* pmeta = nullptr;
  uint32_t *pidx = nullptr, *pcodes = nullptr;
  double* pdict = nullptr;
  int packLevel = 0; // 0 none, 1 16-bit columns, 2 + value dictionary
  int usePacked = 0;
  // spmv_scs64 / spmv_scs64_halo: sixteenths of the reference-layout stream read with plain loads, i.e. kept in the Infinity
  // Cache from one SpMV to the next (sbhip_launch.inc.h: "resident share"); residentRule is what the upload's rule gave
  int residentK = 0, residentRule = 0;
  uint32_t padCol = 0;
  double packedBytes = 0.0; // matrix-stream bytes of the packed form
  uint32_t nWideChunks = 0;
  int nDict = 0;
  // level 3: per-tile x windows staged in LDS
  uint32_t* tileSegPtr = nullptr;
  TileSeg* tileSegs    = nullptr;
  uint32_t* pslots     = nullptr;
  uint32_t ldsWindow   = 0; // doubles, incl. slot 0
  double slotBytes     = 0.0;
  // level 4: pattern dictionary (one byte per element)
  uint16_t* rowBase     = nullptr;
  uint32_t *tileClass = nullptr, *jcodes = nullptr;
  PatEntry* classDict   = nullptr;
  uint32_t* tileHdrs    = nullptr; // TileHdr words: 48 per 4-chunk tile, 128 (two interleaved halves) per 8-chunk tile
  PatEntry* rowPats     = nullptr; // level 5: shared row patterns
  PatEntry* excRows     = nullptr; // level 5: expanded exception rows of the U chunks
  uint32_t patDict = 0, patExcLds = 0; // LDS layout of spmv_scs64_pat: table entries, exception entries
  uint32_t patInterior = 0;            // headers [0, patInterior): tiles that touch no halo column
  // the pattern kernel's tiles: patCPT = 4 or 8 chunks, with their own windows when that differs from level 3's 4
  uint32_t patCPT = 4, patNTiles = 0, patWindow = 0;
  TileSeg* patSegs = nullptr; // == tileSegs when patCPT == 4
  // level 6: the masked form of the same tiles (row programs; usePacked == 5)
  uint32_t* mHdrs    = nullptr; // TileHdr words as tileHdrs; rowPat[] = first block of the chunk's program, exc[] = its padded lanes
  uint32_t* mStream  = nullptr; // code words of its L chunks
  int16_t* mRowBase  = nullptr; // per row: base slot that lines the row up with its chunk's program (may be < 0)
  ProgBlock* mProgs  = nullptr;
  uint32_t mDict = 0, nProgs = 0, nMaskedChunks = 0;
  uint32_t nProgBlocks = 0;      // blocks of 8 entries behind mProgs
  ProgBlockF* mProgsF = nullptr; // single precision with a mirror (sbhip_sp.inc.h): the programs narrowed to float; mProgs is then NULL
  PatEntry* mClassDict = nullptr; // its class tables, windows and segments: the level-5 form's, or its own
  TileSeg* mSegs       = nullptr; // (mOwnsTables) when the windows are laid out in original column order
  uint16_t* mSlotMap   = nullptr; // ... then: [tile][mMapStride] slot -> device column - the 256-slot block's base
  uint32_t mWindow = 0, mMapStride = 0;
  std::vector<uint32_t> mTileOfHdr; // (build time only) which tile the i-th stored header describes
  bool mAllSimple = false;          // every window of the masked form is of the simple kind (<= 6 segments): spmv_prog_fusep
  uint32_t mCPT = 4, mNTiles = 0, mInterior = 0; // its own tile shape (level 5 may have had to take the smaller one)
  bool mOwnsTables = false;
  double mBytes  = 0.0;
  // CRS: a private Sell-64-1 mirror carrying only the pattern levels (SKIPPAD kernel); usePacked
  // 3 = product through the mirror, 0 = native CRS kernel
  sb_matrix* mirror = nullptr;
  uint32_t nRowPats = 0, nUniformChunks = 0;
  uint32_t nPatClasses  = 0;
  double patBytes       = 0.0;
  // single precision (sb_crs_upload_f32 / sb_scs_upload_f32): prec = 1, the values in valf and val == NULL; it streams the
  // reference layout unless the upload built the opt-in float mirror (sb_set_sp_mirror: mProgsF here, or in `mirror` for CRS);
  // no placement tuner
  int prec    = 2; // the reference's PRECISION: 1 single, 2 double
  float* valf = nullptr;
};

// global ids of the halo columns of the matrix about to be uploaded (sb_set_external_ids); consumed by the next upload
static std::vector<uint32_t> g_externalIds;

struct sb_halo {
  uint32_t nr;
  int outdegree, indegree, totalSend, externalCount;
  std::vector<int> destinations, sendCounts, sdispls, sources, recvCounts, rdispls;
  uint32_t* packIdx = nullptr; // device: row (in the vector's order) of each sent element
  double* sendBuf = nullptr;   // device (single precision: the packed floats, or widened to double for a host transport)
  double* recvWide = nullptr;  // device, externalCount doubles: what a host transport delivers to a single-precision exchange
  // exchange over peer-mapped memory (kernels.hip.h: halo_push_k / halo_pull_k); p2p == false: RCCL / transport
  bool p2p = false;
  unsigned long long* stage = nullptr; // own fine-grained area: [2][externalCount] values, then [2][P2P_MAX] flags
  void* peerStage[P2P_MAX] = {};       // destinations' areas as opened here (by destination index)
  HaloPush push;                       // kernel argument of halo_push_k
  HaloPush* dPush = nullptr;           // device copy (the HALO SpMV's push workgroups read it)
  uint32_t *slot = nullptr; uint8_t* dest = nullptr; unsigned int* done = nullptr; // device arrays behind `push`
  int *dSrcRank = nullptr, *dRdispl = nullptr, *dRcount = nullptr, *err = nullptr;
  unsigned long long seq = 0;
  char p2pReason[256] = "not set up";
  // the exchange folded into the streaming loop's kernels (sb_comm_halo_fold; kernels.hip.h: cg_update_p_push, spmv_scs64_halo).
  // Built by the first folded solve (sbhip_comm.inc.h: halo_fold_send_plan / halo_fold_block_plan), freed by halo_p2p_release.
  std::vector<uint32_t> hPackIdx, hSlot; // host copies of packIdx / slot / dest as the push kernels use them
  std::vector<uint8_t> hDest;
  struct FoldSend {                      // the send list sorted by owning workgroup of the p update's grid, per precision
    uint32_t grid = 0, vb = 0;           // the grid it was built for
    HaloFold fold = {};
    uint32_t *row = nullptr, *slot = nullptr, *wgStart = nullptr;
    uint8_t* dest = nullptr;
  } foldSend[2];                         // [0] fp64 (two rows per thread and step), [1] fp32 (four)
  const sb_matrix* foldMatrix = nullptr; // the matrix the block split below was made for
  uint32_t foldChunks = 0, foldInterior = 0;
  uint32_t* foldOrder = nullptr;         // device: interior 4-chunk blocks ascending, then the halo blocks (ScsHalo::order)
};

struct sb_cg {
  const sb_matrix* A;
  sb_halo* halo;
  uint32_t nr, nc;
  double *r, *p, *Ap, *x, *b, *xexact;
  // p double-buffered for the SpMV that takes the p update (pack.hip.h: spmv_prog_fusep): body k reads pbuf[(k-1) & 1] and
  // writes pbuf[k & 1]; pbuf[0] == p
  double* pbuf[2] = { nullptr, nullptr };
  char* vecSlab = nullptr; // the loop's vectors live in ONE allocation, `vecPad` bytes apart (sb_cg_create)
  size_t vecPad = 0, vecSlabBytes = 0;
  bool vecFromArena = false; // the vectors sit in the matrix's tuned arena (sb_matrix::vecArena), not in an allocation of their own
  int fusepPlan = -1; // 1: the loop uses spmv_prog_fusep, 0: not, -1: not decided yet
  int fusepWant = -1; // sb_cg_set_fuse_p: 1 / 0, -1: SB_FUSE_P or the library default
  int fusepLatched = -1; // the plan of the solve that is running (set by sb_cg_start, cleared by sb_cg_finish)
  int fuseAlphaWant = -1; // sb_cg_set_fuse_alpha: 1 / 0, -1: SB_FUSE_ALPHA or the library default (on)
  int fuseBetaWant  = -1; // sb_cg_set_fuse_beta
  int betaFold      = 0;  // 1 / 2: the last enqueued body left its beta step to the next p update (fold mode)
  int fusedWant     = 1;  // sb_cg_set_fused: the caller's level; `fused` is what runs (0 while the dot order is seq)
  int dotOrderWant  = -1; // sb_cg_set_dot_order: 0 tree / 1 seq, -1: the process default (sb_dot_order)
  int seqLatched    = -1; // the dot order of the solve that is running (set by sb_cg_start, cleared by sb_cg_finish)
  int foldLatched   = -1; // the halo-fold plan of the solve that is running (halo_fold_plan; same life)
  CgScalars* S;
  double* partials;
  uint32_t nPartials;
  double *rr_hist, *pAp_hist;
  int hist_cap;
  int fused;
  double region_ms[4];
  std::vector<hipEvent_t> ev;
  std::vector<int> evRegion;
  size_t evUsed;
  bool timing;
  hipEvent_t evLoop0, evLoop1;
  float loop_ms;
  // optional in-situ timing of every SpMV launch (bench.py's roofline leg)
  bool spmvTiming;
  std::vector<hipEvent_t> spmvEv;
  size_t spmvEvUsed;
  // optional event after every launch of the loop (bench.py's per-kernel breakdown): phase_mark() in sbhip_cg.inc.h
  bool phaseTiming = false;
  std::vector<hipEvent_t> phEv;
  std::vector<int> phId;
  size_t phUsed = 0;
  int k_next;        // next loop body to enqueue
  bool started;
  CgScalars hostS;   // staging copy for the H2D of the control block
  double* partials2 = nullptr; // level-0 partials of r.r (the p.Ap ones stay in `partials` while it reads them)
  // single precision (sb_cg_create_f32; sbhip_sp.inc.h): prec = 1 and the loop's state below; the double members stay NULL
  int prec = 2;
  float* pf2 = nullptr; // the second p buffer of the fused p update (spmv_prog_fusep_f32): body k reads buffer (k-1) & 1, writes k & 1; pf is buffer 0
  float *rf = nullptr, *pf = nullptr, *Apf = nullptr, *xf = nullptr, *bf = nullptr, *xexactf = nullptr;
  CgScalarsF* SF = nullptr;
  float *partialsF = nullptr, *partials2F = nullptr, *rrHistF = nullptr, *pApHistF = nullptr;
  CgCommF* XF = nullptr; // several ranks: the rank sum handed to the all-reduce, the peer-mapped plane's failure flag
};

// ===========================================================================
// context
// ===========================================================================
// Every sb_* function below is declared extern "C" by include/sbhip.h, which fixes
// its linkage; the helpers in between stay C++.

const char* sb_version(void) { return "sparsebench_amd sbhip 0.5 (gfx950)"; }
int sb_lab_build(void) { return 0; } // (there is one build: DESIGN 4.6)

int sb_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void sb_init(int device)
{
  if (g.init) {
    if (device != g.device) SB_FATAL("already initialised on device %d", g.device);
    return;
  }
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0)
    SB_FATAL("no HIP device visible (%s): the HIP path is the only path", hipGetErrorString(e));
  if (device < 0 || device >= n) SB_FATAL("device %d out of range (%d visible)", device, n);
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipGetDeviceProperties(&g.prop, device));
  snprintf(g.name, sizeof g.name, "%s (%s)", g.prop.name[0] ? g.prop.name : "AMD Instinct", g.prop.gcnArchName);
  HIP_CHECK(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
  HIP_CHECK(hipMalloc(&g.scalar, 64));
  HIP_CHECK(hipMemset(g.scalar, 0, 64)); // [0] scratch double, [4] a permanent int 0 (zero_flag)
  g.device = device;
  g.init   = true;
  g.pushInside = getenv("SB_HALO_PUSH_INSIDE") && atoi(getenv("SB_HALO_PUSH_INSIDE")) != 0;
}

void sb_finalize(void)
{
  if (!g.init) return;
  HIP_CHECK(hipStreamSynchronize(g.stream));
  if (g.comm) sb_comm_finalize();
  if (g.partials) HIP_CHECK(hipFree(g.partials));
  for (int i = 0; i < 2; i++)
    if (g.ws[i]) HIP_CHECK(hipFree(g.ws[i]));
  HIP_CHECK(hipFree(g.scalar));
  HIP_CHECK(hipStreamDestroy(g.stream));
  g = Ctx();
}

int sb_is_initialized(void) { return g.init ? 1 : 0; }
const char* sb_device_name(void) { need_init(); return g.name; }
int sb_num_cus(void) { need_init(); return g.prop.multiProcessorCount; }
void sb_sync(void) { need_init(); HIP_CHECK(hipStreamSynchronize(g.stream)); }
void* sb_stream(void) { need_init(); return (void*)g.stream; }

void* sb_malloc(size_t bytes)
{
  need_init();
  void* p = nullptr;
  HIP_CHECK(hipMalloc(&p, bytes ? bytes : 8));
  return p;
}
void sb_free(void* dev)
{
  if (dev) HIP_CHECK(hipFree(dev));
}
void sb_memset(void* dev, int byte, size_t bytes)
{
  need_init();
  HIP_CHECK(hipMemsetAsync(dev, byte, bytes, g.stream));
}
// Host <-> device copies through this layer are counted (sb_copy_counters): the drop-in's claim "the reference's own -t spmv loop
// moves nothing over PCIe"  is asserted on these counters by tests/test_gpu_dropin.py.
static uint64_t g_copies[4]; // h2d calls, h2d bytes, d2h calls, d2h bytes
void sb_h2d(void* dev, const void* host, size_t bytes)
{
  need_init();
  g_copies[0]++, g_copies[1] += bytes;
  HIP_CHECK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, g.stream));
  HIP_CHECK(hipStreamSynchronize(g.stream));
}
void sb_d2h(void* host, const void* dev, size_t bytes)
{
  need_init();
  g_copies[2]++, g_copies[3] += bytes;
  HIP_CHECK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, g.stream));
  HIP_CHECK(hipStreamSynchronize(g.stream));
}
void sb_copy_counters(uint64_t out[4])
{
  for (int i = 0; i < 4; i++) out[i] = g_copies[i];
}

// ---- host-visible device memory: the reference's allocation hook -------------------------------------------------------
// src/allocate.c:12-36 hands out the vectors that src/main.c:205-211 fills with HOST loops and then passes to spMVM
// (src/main.c:213-215).  For that loop to time the kernel and not PCIe staging, allocate() (host/sbh_base.c) asks here for
// memory that lives in HBM, that the CPU can store to through the PCIe BAR, and that kernels read in place: fine-grained
// device memory (hipDeviceMallocFinegrained: device accesses stay coherent with the host's stores; a coarse-grained hipMalloc
// region may be served from a stale L2 line after a host store).  Whether the CPU can really reach it is PROBED once, with the
// store guarded by a SIGSEGV / SIGBUS handler: a box without a large BAR answers with a fault, not with an error code.
static struct HostVisible {
  int probed = 0, ok = 0;
  char reason[320] = "not probed yet";
} hv;
static sigjmp_buf hv_jmp;
static void hv_fault(int) { siglongjmp(hv_jmp, 1); }

static bool hv_guarded_cpu_roundtrip(volatile uint64_t* p, uint64_t v)
{
  struct sigaction sa, oldSegv, oldBus;
  memset(&sa, 0, sizeof sa);
  sa.sa_handler = hv_fault;
  sigemptyset(&sa.sa_mask);
  sigaction(SIGSEGV, &sa, &oldSegv);
  sigaction(SIGBUS, &sa, &oldBus);
  bool ok = false;
  if (sigsetjmp(hv_jmp, 1) == 0) {
    p[0] = v;
    __sync_synchronize();
    ok = p[0] == v;
  }
  sigaction(SIGSEGV, &oldSegv, nullptr);
  sigaction(SIGBUS, &oldBus, nullptr);
  return ok;
}

static void hv_probe(void)
{
  hv.probed = 1;
  const char* off = getenv("SPARSEBENCH_ALLOCATE");
  if (off && strcmp(off, "host") == 0) {
    snprintf(hv.reason, sizeof hv.reason, "SPARSEBENCH_ALLOCATE=host: allocate() hands out plain host memory (vectors are staged)");
    return;
  }
  int largeBar = 0;
  if (hipDeviceGetAttribute(&largeBar, hipDeviceAttributeIsLargeBar, g.device) != hipSuccess) (void)hipGetLastError();
  void* p = nullptr;
  hipError_t e = hipExtMallocWithFlags(&p, 4096, hipDeviceMallocFinegrained);
  if (e != hipSuccess || !p) {
    (void)hipGetLastError();
    snprintf(hv.reason, sizeof hv.reason, "hipExtMallocWithFlags(hipDeviceMallocFinegrained) failed: %s (large BAR attribute: %d)",
        hipGetErrorString(e), largeBar);
    return;
  }
  const uint64_t v = 0x5b5b00c0ffee1234ull;
  if (!hv_guarded_cpu_roundtrip((volatile uint64_t*)p, v)) {
    snprintf(hv.reason, sizeof hv.reason, "the CPU cannot store to fine-grained device memory on this box (fault or wrong read-back; "
        "large BAR attribute: %d)", largeBar);
    (void)hipFree(p);
    return;
  }
  // the device must see the host's store, and the host the device's
  uint64_t back = 0;
  bool ok = hipMemcpy(&back, p, 8, hipMemcpyDeviceToHost) == hipSuccess && back == v;
  ok = ok && hipMemset(p, 0x3c, 8) == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
       *(volatile uint64_t*)p == 0x3c3c3c3c3c3c3c3cull;
  (void)hipFree(p);
  if (!ok) {
    (void)hipGetLastError();
    snprintf(hv.reason, sizeof hv.reason, "host stores to fine-grained device memory did not reach the device (or the other way round)");
    return;
  }
  hv.ok = 1;
  snprintf(hv.reason, sizeof hv.reason, "fine-grained device memory, CPU-writable through the PCIe BAR (probed: host store -> device "
      "read, device store -> host read; large BAR attribute: %d)", largeBar);
}

void* sb_malloc_host_visible(size_t bytes)
{
  need_init();
  if (!hv.probed) hv_probe();
  if (!hv.ok) return nullptr;
  void* p = nullptr;
  if (hipExtMallocWithFlags(&p, bytes ? bytes : 8, hipDeviceMallocFinegrained) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}
const char* sb_host_visible_reason(void)
{
  if (g.init && !hv.probed) hv_probe();
  return hv.reason;
}
void* sb_malloc_pinned_host(size_t bytes)
{
  need_init();
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 8, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}
void sb_free_pinned_host(void* p)
{
  if (p) HIP_CHECK(hipHostFree(p));
}
int sb_is_pinned_host_ptr(const void* p)
{
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return a.type == hipMemoryTypeHost ? 1 : 0;
}
size_t sb_mem_free_bytes(void)
{
  need_init();
  size_t freeB = 0, totalB = 0;
  HIP_CHECK(hipMemGetInfo(&freeB, &totalB));
  return freeB;
}

// ---- device-timed profile regions (PROFILE macro, src/profiler.h:18-21) ---------------------------------------------------
// The reference's PROFILE reads the host clock around a synchronous CPU call.  Here the call is a stream-ordered launch: a
// region is bracketed by two events on the layer's stream (no system-scope fence), nothing waits inside the loop, and the
// accumulated DEVICE time is read when the table is printed ("time regions with hipEvents and fill _t[] afterwards").
struct RegionTimer {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> open; // recorded, not yet read
  std::vector<hipEvent_t> spare;
  double seconds = 0.0;
  uint64_t count = 0;
  hipEvent_t cur = nullptr;
};
static RegionTimer g_regions[8];
static hipEvent_t region_event(RegionTimer& r)
{
  if (!r.spare.empty()) {
    hipEvent_t e = r.spare.back();
    r.spare.pop_back();
    return e;
  }
  hipEvent_t e;
  HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
  return e;
}
static void region_drain(RegionTimer& r, size_t keep)
{
  while (r.open.size() > keep) {
    auto pr = r.open.front();
    float ms = 0.f;
    HIP_CHECK(hipEventSynchronize(pr.second));
    HIP_CHECK(hipEventElapsedTime(&ms, pr.first, pr.second));
    r.seconds += 1e-3 * ms;
    r.spare.push_back(pr.first), r.spare.push_back(pr.second);
    r.open.erase(r.open.begin());
  }
}
void sb_region_begin(int tag)
{
  if (!g.init || tag < 0 || tag >= 8) return;
  RegionTimer& r = g_regions[tag];
  r.cur          = region_event(r);
  HIP_CHECK(hipEventRecord(r.cur, g.stream));
}
void sb_region_end(int tag)
{
  if (!g.init || tag < 0 || tag >= 8 || !g_regions[tag].cur) return;
  RegionTimer& r = g_regions[tag];
  hipEvent_t e   = region_event(r);
  HIP_CHECK(hipEventRecord(e, g.stream));
  r.open.push_back({ r.cur, e });
  r.cur = nullptr;
  r.count++;
  if (r.open.size() >= 512) region_drain(r, 256); // (the oldest are long complete: no stall in practice)
}
double sb_region_seconds(int tag, uint64_t* count)
{
  if (tag < 0 || tag >= 8) return 0.0;
  RegionTimer& r = g_regions[tag];
  if (g.init) region_drain(r, 0);
  if (count) *count = r.count;
  return r.seconds;
}
void sb_region_reset(void)
{
  for (auto& r : g_regions) {
    if (g.init) region_drain(r, 0);
    r.seconds = 0.0, r.count = 0;
  }
}
void sb_d2d(void* dst, const void* src, size_t bytes)
{
  need_init();
  HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, g.stream));
}
int sb_is_device_ptr(const void* p)
{
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return a.type == hipMemoryTypeDevice ? 1 : 0;
}

void* sb_event_create(void)
{
  need_init();
  hipEvent_t e;
  HIP_CHECK(hipEventCreate(&e));
  return (void*)e;
}
void sb_event_record(void* ev) { HIP_CHECK(hipEventRecord((hipEvent_t)ev, g.stream)); }
float sb_event_elapsed_ms(void* a, void* b)
{
  float ms = 0.f;
  HIP_CHECK(hipEventSynchronize((hipEvent_t)b));
  HIP_CHECK(hipEventElapsedTime(&ms, (hipEvent_t)a, (hipEvent_t)b));
  return ms;
}
void sb_event_destroy(void* ev) { HIP_CHECK(hipEventDestroy((hipEvent_t)ev)); }

// The rest of the layer, in reading order (one translation unit: one hipcc call, one .so):
#include "sbhip_matrix.inc.h"
#include "sbhip_launch.inc.h"
#include "sbhip_comm.inc.h"
#include "sbhip_solver.inc.h"
#include "sbhip_cg.inc.h"
#include "sbhip_sp.inc.h"
#include "sbhip_gmres.inc.h"
#include "sbhip_cgb.inc.h"
#include "sbhip_pcg.inc.h"
#include "sbhip_sgs.inc.h"
#include "sbhip_poly.inc.h"
#include "sbhip_mg.inc.h"
#include "sbhip_mg_fw.inc.h"
#include "sbhip_precond.inc.h"
#include "sbhip_galerkin.inc.h"
#include "sbhip_aggregation.inc.h"
#include "sbhip_pcg_loop.inc.h"
#include "sbhip_bicgstab.inc.h"
#include "sbhip_gmres_precond.inc.h"
