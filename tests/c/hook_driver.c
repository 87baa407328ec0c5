/* hook_driver.c -- a caller written ONLY against the reference-shaped API (include/sparsebench/sparsebench.h) whose vectors
 * all come from allocate(), at sizes where the hook hands out memory that lives in HBM.  It uses them the way the reference's
 * callers use host memory: fill by host loops, call, read the output on return, refill an input on return.  Values are printed
 * with %a for the pytest side (tests/test_gpu_hook_vectors.py) to compare bit for bit.  Built with -DCRS and -DSCS, each in
 * double and with -DPRECISION=1.
 *
 *   hook_driver nx ny nz K [sync] [nomixed]
 *       the sequence below; K = spMVM calls queued ahead of each checked one, so that a call which only enqueued its kernel is
 *       K kernels away from its result when the host looks.
 *       sync: the caller waits (sbh_profile_sync) after each checked call, before it touches a vector -- what spMVM / waxpby on
 *       hook vectors ask of their caller today (sparsebench.h).  WITHOUT it this is the reference-shaped caller proper, which
 *       never synchronises: it reads NaN sentinels in steps 3, 4 and 6 until those calls wait for their kernels themselves.
 *       nomixed leaves step 9 out (the test counts step 9's copies as the difference).
 *   hook_driver table
 *       300 live requests of 64 KiB, more than the 256 the hook's table once held
 */
#include <math.h>
#include <stdlib.h>

#include "sparsebench/sparsebench.h"

static CG_FLOAT* snap; /* plain host memory, taken before any call */
static int caller_syncs;

/* after a checked call, before the host touches a vector */
static void settle(void)
{
  if (caller_syncs) sbh_profile_sync();
}

/* read v[n-1] down to v[0] at once -- the end of the vector first, the part a kernel still in flight writes last -- then print */
static void dump(const char* tag, const volatile CG_FLOAT* v, CG_UINT n)
{
  for (CG_UINT i = n; i-- > 0;) snap[i] = v[i];
  for (CG_UINT i = 0; i < n; i++) printf("%s %u %a\n", tag, i, (double)snap[i]);
}

static void fill_a(CG_FLOAT* x, CG_UINT n)
{
  for (CG_UINT i = 0; i < n; i++) x[i] = 1.0 + 0.001 * (double)(i % 97);
}

static void fill_b(CG_FLOAT* x, CG_UINT n)
{
  for (CG_UINT i = 0; i < n; i++) x[i] = 2.0 - 0.003 * (double)(i % 89);
}

static void fill_nan(CG_FLOAT* x, CG_UINT n)
{
  for (CG_UINT i = 0; i < n; i++) x[i] = NAN;
}

static CG_FLOAT* hook_vector(const char* name, CG_UINT n)
{
  CG_FLOAT* p = (CG_FLOAT*)allocate(ARRAY_ALIGNMENT, n * sizeof(CG_FLOAT));
  printf("kind %s %d\n", name, sbh_allocate_kind());
  return p;
}

static int table_mode(void)
{
  enum { N = 300 };
  const size_t bytes = (size_t)64 << 10;
  static volatile CG_FLOAT* p[N];
  printf("free before %zu\n", sbh_device_free_bytes());
  for (int i = 0; i < N; i++) {
    p[i] = (volatile CG_FLOAT*)allocate(ARRAY_ALIGNMENT, bytes);
    if (i == 0 || i == N - 1) printf("kind %d %d\n", i, sbh_allocate_kind());
  }
  int bad = 0;
  for (int i = 0; i < N; i++) p[i][0] = (CG_FLOAT)(i + 1);
  for (int i = 0; i < N; i++) bad += p[i][0] != (CG_FLOAT)(i + 1);
  printf("free held %zu\n", sbh_device_free_bytes());
  for (int i = 0; i < N; i++) sbh_allocate_free((void*)p[i]);
  printf("free after %zu\n", sbh_device_free_bytes());
  printf("readback mismatches %d\n", bad);
  return bad;
}

int main(int argc, char** argv)
{
  Comm comm;
  Parameter param;
  commInit(&comm, argc, argv);
  if (argc == 2 && strcmp(argv[1], "table") == 0) {
    const int bad = table_mode();
    commFinalize(&comm);
    return bad ? EXIT_FAILURE : EXIT_SUCCESS;
  }
  if (argc < 5) {
    fprintf(stderr, "usage: %s nx ny nz K [sync] [nomixed] | %s table\n", argv[0], argv[0]);
    return EXIT_FAILURE;
  }
  initParameter(&param);
  param.nx = atoi(argv[1]), param.ny = atoi(argv[2]), param.nz = atoi(argv[3]);
  const int K     = atoi(argv[4]);
  int mixed       = 1;
  for (int i = 5; i < argc; i++) {
    if (strcmp(argv[i], "sync") == 0) caller_syncs = 1;
    if (strcmp(argv[i], "nomixed") == 0) mixed = 0;
  }
  GMatrix m;
  matrixGenerate(&m, &param, comm.rank, comm.size, false);
  commPartition(&comm, &m);
  Matrix sm;
  memset(&sm, 0, sizeof sm);
#ifdef SCS
  sm.C = 64, sm.sigma = 128;
#endif
  convertMatrix(&sm, &m);
  const CG_UINT nr = m.nr, nc = m.nc;
  snap             = (CG_FLOAT*)malloc((size_t)nc * sizeof(CG_FLOAT));
  CG_FLOAT* xm     = (CG_FLOAT*)malloc((size_t)nc * sizeof(CG_FLOAT));
  CG_FLOAT* ym     = (CG_FLOAT*)malloc((size_t)nr * sizeof(CG_FLOAT));

  /* 1, 2 */
  CG_FLOAT* x  = hook_vector("x", nc);
  CG_FLOAT* y  = hook_vector("y", nr);
  CG_FLOAT* y2 = hook_vector("y2", nr);
  CG_FLOAT* w  = hook_vector("w", nr);
  fill_a(x, nc);
  fill_nan(y, nr), fill_nan(y2, nr), fill_nan(w, nr);

  /* 3: read after call, with work queued ahead */
  for (int k = 0; k < K; k++) spMVM(&sm, x, y2);
  spMVM(&sm, x, y);
  settle();
  dump("s3", y, nr);

  /* 4: refill after call */
  fill_nan(y, nr);
  for (int k = 0; k < K; k++) spMVM(&sm, x, y2);
  spMVM(&sm, x, y);
  settle();
  fill_nan(x, nc);
  fill_a(x, nc);
  dump("s4", y, nr);

  /* 5: store then call */
  fill_b(x, nc);
  spMVM(&sm, x, y);
  settle();
  dump("s5", y, nr);

  /* 6, 7: waxpby, then with the output aliasing an input */
  waxpby(nr, 1.0, y, -0.5, x, w);
  settle();
  dump("s6", w, nr);
  waxpby(nr, 2.0, w, 1.0, y, w);
  settle();
  dump("s7w", w, nr);
  waxpby(nr, 1.0, x, -2.0, y, x);
  settle();
  dump("s7x", x, nr);

  /* 8 */
  CG_FLOAT d1 = 0.0, d2 = 0.0;
  ddot(nr, w, y, &d1);
  ddot(nr, y, y, &d2);
  printf("dot %a %a\n", (double)d1, (double)d2);

  /* 9: mixed operands -- one vector of each call is plain host memory and is staged */
  if (mixed) {
    fill_nan(ym, nr);
    spMVM(&sm, x, ym);
    settle();
    dump("s9a", ym, nr);
    fill_a(xm, nc);
    fill_nan(y, nr);
    spMVM(&sm, xm, y);
    settle();
    dump("s9b", y, nr);
    fill_nan(w, nr);
    waxpby(nr, 1.0, xm, -0.5, y, w);
    settle();
    dump("s9c", w, nr);
  }

  /* 10 */
  sbh_allocate_free(x), sbh_allocate_free(y), sbh_allocate_free(y2), sbh_allocate_free(w);
  free(xm), free(ym), free(snap);
  commFinalize(&comm);
  return EXIT_SUCCESS;
}
