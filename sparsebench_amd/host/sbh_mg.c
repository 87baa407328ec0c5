/* sbh_mg.c -- the geometric hierarchy of a generated matrix for the multigrid preconditioner of PCG: how deep the
 * grid lets it go, the injection maps, and the coarse levels themselves: the stencil regenerated on each coarser grid through
 * the same calls the driver makes for the fine one (generate -> commPartition -> convert).  solvePCGMG's body (sbh_solver.c)
 * hands them to sb_pcg_create_mg -- or, with the trilinear prolongations below in the injection maps' place, to
 * sb_pcg_create_mg_p.  Nothing is computed here but those weights, products of 1 and 1/2.
 */
#define _GNU_SOURCE
#include <stdint.h>
#include <stdlib.h>

#include "sbhip.h"
#include "sparsebench/sparsebench.h"

#define MG_AUTO_DEPTH 4 /* HPCG's */

static int divisible(int n, int by) { return n > 0 && n % by == 0; }

int sbh_mg_levels(int nx, int ny, int nz, int want, char* why, size_t cap)
{
  if (why && cap) why[0] = '\0';
  if (want < 0) {
    if (why) snprintf(why, cap, "MG: %d levels asked for (1 or more, or 0 for the deepest of up to %d)", want, MG_AUTO_DEPTH);
    return 0;
  }
  if (nx < 1 || ny < 1 || nz < 1) {
    if (why) snprintf(why, cap, "MG: the grid %d x %d x %d has an empty dimension", nx, ny, nz);
    return 0;
  }
  const int top = want ? want : MG_AUTO_DEPTH;
  for (int L = top; L >= 1; L--) {
    const int f = L < 31 ? 1 << (L - 1) : 0;
    const int div = f && divisible(nx, f) && divisible(ny, f) && divisible(nz, f);
    const int big = L == 1 || (div && nx / f >= 2 && ny / f >= 2 && nz / f >= 2);
    if (div && big) return L;
    if (want) {
      if (!why) return 0;
      if (!f) snprintf(why, cap, "MG: %d levels are more than any grid allows", L);
      else if (!div) snprintf(why, cap, "MG: %d levels need every dimension divisible by %d (the grid is %d x %d x %d)", L, f, nx, ny, nz);
      else
        snprintf(why, cap, "MG: %d levels would give a coarse dimension smaller than 2 (the grid is %d x %d x %d, the coarsest %d x %d x %d)",
            L, nx, ny, nz, nx / f, ny / f, nz / f);
      return 0;
    }
  }
  return 1;
}

void sbh_mg_f2c(int nx, int ny, int nz, CG_UINT* f2c)
{
  const int cx = nx / 2, cy = ny / 2, cz = nz / 2;
  for (int z = 0; z < cz; z++)
    for (int y = 0; y < cy; y++)
      for (int x = 0; x < cx; x++)
        f2c[((size_t)z * cy + y) * cx + x] = (CG_UINT)(((size_t)(2 * z) * ny + 2 * y) * nx + 2 * x);
}

/* the trilinear prolongation (sparsebench.h): per dimension an even fine index i takes coarse i / 2 with weight 1, an odd one
 * (i - 1) / 2 and (i + 1) / 2 with 1/2 each, the second dropped where it is past the coarse grid; a row's weights are the
 * products, its entries in ascending coarse number */
static int line_weights(int i, int nc, int idx[2], double w[2])
{
  if (i % 2 == 0) {
    idx[0] = i / 2, w[0] = 1.0;
    return 1;
  }
  idx[0] = (i - 1) / 2, w[0] = 0.5;
  idx[1] = (i + 1) / 2, w[1] = 0.5;
  return idx[1] < nc ? 2 : 1;
}

void sbh_mg_trilinear(int nx, int ny, int nz, uint64_t* ptr, CG_UINT* col, double* val)
{
  const int cx = nx / 2, cy = ny / 2, cz = nz / 2;
  uint64_t o = 0;
  size_t row = 0;
  ptr[0]     = 0;
  for (int z = 0; z < nz; z++)
    for (int y = 0; y < ny; y++)
      for (int x = 0; x < nx; x++) {
        int ix[2], iy[2], iz[2];
        double wx[2], wy[2], wz[2];
        const int kx = line_weights(x, cx, ix, wx), ky = line_weights(y, cy, iy, wy), kz = line_weights(z, cz, iz, wz);
        for (int c = 0; c < kz; c++)
          for (int b = 0; b < ky; b++)
            for (int a = 0; a < kx; a++) {
              col[o] = (CG_UINT)(((size_t)iz[c] * cy + iy[b]) * cx + ix[a]);
              val[o] = wz[c] * wy[b] * wx[a];
              o++;
            }
        ptr[++row] = o;
      }
}

/* one coarse level: the generator's matrix on its grid, converted and uploaded as the fine one was */
typedef struct {
  GMatrix gm;
  CRSMatrix crs;
  SCSMatrix scs;
  void* dev;
  CG_UINT* f2c; /* from the level above */
  /* Galerkin mode: the prolongation from this level (owned here, handed to the solver handle's constructor) */
  uint64_t* pptr;
  CG_UINT* pcol;
  double* pval;
} mg_level;

static void level_free(mg_level* v, int fmt)
{
  if (v->dev) sb_matrix_free((sb_matrix*)v->dev);
  free(v->gm.rowPtr), free(v->gm.entries), free(v->f2c);
  free(v->pptr), free(v->pcol), free(v->pval);
  if (fmt == 0) free(v->crs.rowPtr), free(v->crs.colInd), free(v->crs.val), free(v->crs.rowNnz);
  else
    free(v->scs.chunkPtr), free(v->scs.chunkLens), free(v->scs.colInd), free(v->scs.val), free(v->scs.oldToNewPerm),
        free(v->scs.newToOldPerm), free(v->scs.rowNnz);
}

/* the coarse levels (sparsebench.h) */
void* sbh_mg_hierarchy_build(const Parameter* param, int fmt, CG_UINT C, CG_UINT sigma, int L, const void** mats, const CG_UINT** maps)
{
  mg_level* lev = (mg_level*)calloc((size_t)L + 1, sizeof *lev);
  Parameter pc  = *param;
  for (int l = 1; l < L; l++) {
    mg_level* v = &lev[l];
    v->f2c      = (CG_UINT*)malloc(((size_t)(pc.nx / 2) * (pc.ny / 2) * (pc.nz / 2) + 1) * sizeof(CG_UINT));
    sbh_mg_f2c(pc.nx, pc.ny, pc.nz, v->f2c);
    pc.nx /= 2, pc.ny /= 2, pc.nz /= 2;
    Comm cc;
    memset(&cc, 0, sizeof cc);
    cc.size = 1;
    sbh_init_matrix(&cc, &pc, &v->gm);
    commPartition(&cc, &v->gm);
    if (fmt == 0) {
      sbh_convert_crs(&v->crs, &v->gm);
      v->dev = v->crs.dev;
    } else {
      v->scs.C = C, v->scs.sigma = sigma;
      sbh_convert_scs(&v->scs, &v->gm);
      v->dev = v->scs.dev;
    }
    mats[l - 1] = v->dev, maps[l - 1] = v->f2c;
  }
  return lev;
}

/* a one-rank GMatrix from CSR in memory (sparsebench.h): what MMMatrixRead -> matrixConvertfromMM make of the same entries in a
 * file -- a row's entries in ascending column, storage order kept among equal columns */
void sbh_gmatrix_from_csr(GMatrix* m, CG_UINT n, const uint64_t* ptr, const CG_UINT* col, const double* val)
{
  const uint64_t nnz = ptr[n];
  if (ptr[0] != 0 || nnz > 0xFFFFFFFEull) {
    fprintf(stderr, "sbh_gmatrix_from_csr: row pointers from %llu to %llu: must start at 0 and fit the 32-bit row pointer\n",
        (unsigned long long)ptr[0], (unsigned long long)nnz);
    exit(EXIT_FAILURE);
  }
  memset(m, 0, sizeof *m);
  m->nr = m->nc = m->totalNr = n;
  m->nnz = m->totalNnz = (CG_UINT)nnz;
  m->startRow = 0, m->stopRow = n ? n - 1 : 0;
  m->entries  = (Entry*)sbh_alloc_host(ARRAY_ALIGNMENT, ((size_t)nnz + 1) * sizeof(Entry));
  m->rowPtr   = (CG_UINT*)sbh_alloc_host(ARRAY_ALIGNMENT, ((size_t)n + 1) * sizeof(CG_UINT));
  m->rowPtr[0] = 0;
  for (CG_UINT i = 0; i < n; i++) {
    if (ptr[i + 1] < ptr[i]) {
      fprintf(stderr, "sbh_gmatrix_from_csr: the row pointer falls at row %u\n", i);
      exit(EXIT_FAILURE);
    }
    m->rowPtr[i + 1] = (CG_UINT)ptr[i + 1];
    for (uint64_t q = ptr[i]; q < ptr[i + 1]; q++) {
      if (col[q] >= n) {
        fprintf(stderr, "sbh_gmatrix_from_csr: row %u has column %u outside the %u rows\n", i, col[q], n);
        exit(EXIT_FAILURE);
      }
      uint64_t o = q; /* stable insertion by column: rows are short and usually sorted already */
      for (; o > ptr[i] && m->entries[o - 1].col > col[q]; o--) m->entries[o] = m->entries[o - 1];
      m->entries[o].col = col[q], m->entries[o].val = (CG_FLOAT)val[q];
    }
  }
}

/* the coarse levels as Galerkin products formed on the device (sparsebench.h) */
void* sbh_mg_hierarchy_build_galerkin(const Parameter* param, const void* fine_dev, int fmt, CG_UINT C, CG_UINT sigma, int L,
    const void** mats, const uint64_t** p_ptr, const CG_UINT** p_col, const double** p_val, double* stage_ms)
{
#if PRECISION == 1
  (void)param, (void)fine_dev, (void)fmt, (void)C, (void)sigma, (void)L, (void)mats, (void)p_ptr, (void)p_col, (void)p_val, (void)stage_ms;
  fprintf(stderr, "MG: the Galerkin hierarchy is double precision only\n");
  exit(EXIT_FAILURE);
#else
  mg_level* lev = (mg_level*)calloc((size_t)L + 1, sizeof *lev);
  int nx = param->nx, ny = param->ny, nz = param->nz;
  const void* fine = fine_dev;
  for (int l = 1; l < L; l++) {
    mg_level* v    = &lev[l];
    const size_t n = (size_t)nx * ny * nz;
    v->pptr = (uint64_t*)malloc((n + 1) * sizeof(uint64_t)), v->pcol = (CG_UINT*)malloc(8 * n * sizeof(CG_UINT));
    v->pval = (double*)malloc(8 * n * sizeof(double));
    sbh_mg_trilinear(nx, ny, nz, v->pptr, v->pcol, v->pval);
    nx /= 2, ny /= 2, nz /= 2;
    const CG_UINT nc = (CG_UINT)((size_t)nx * ny * nz);
    sb_csr* ac       = sb_matrix_galerkin((const sb_matrix*)fine, nc, v->pptr, v->pcol, v->pval);
    const uint64_t nnz = sb_csr_nnz(ac);
    uint64_t* ptr    = (uint64_t*)malloc(((size_t)nc + 1) * sizeof(uint64_t));
    CG_UINT* col     = (CG_UINT*)malloc((nnz + 1) * sizeof(CG_UINT));
    double* val      = (double*)malloc((nnz + 1) * sizeof(double));
    double st[6];
    sb_csr_copy(ac, ptr, col, val), sb_csr_stats(ac, st), sb_csr_free(ac);
    if (stage_ms) stage_ms[2 * (l - 1)] = st[0], stage_ms[2 * (l - 1) + 1] = st[1];
    sbh_gmatrix_from_csr(&v->gm, nc, ptr, col, val);
    free(ptr), free(col), free(val);
    Comm cc;
    memset(&cc, 0, sizeof cc);
    cc.size = 1;
    commPartition(&cc, &v->gm);
    if (fmt == 0) {
      sbh_convert_crs(&v->crs, &v->gm);
      v->dev = v->crs.dev;
    } else {
      v->scs.C = C, v->scs.sigma = sigma;
      sbh_convert_scs(&v->scs, &v->gm);
      v->dev = v->scs.dev;
    }
    mats[l - 1] = v->dev, p_ptr[l - 1] = v->pptr, p_col[l - 1] = v->pcol, p_val[l - 1] = v->pval;
    fine = v->dev;
  }
  return lev;
#endif
}

/* the coarse levels by smoothed aggregation from the matrix alone (sparsebench.h) */
void* sbh_mg_hierarchy_build_sa(const void* fine_dev, CG_UINT fine_nr, int fmt, CG_UINT C, CG_UINT sigma, int maxL, double theta,
    double omega_s, int* L_out, const void** mats, const uint64_t** p_ptr, const CG_UINT** p_col, const double** p_val, CG_UINT* rows,
    CG_UINT* rounds, double* ms)
{
#if PRECISION == 1
  (void)fine_dev, (void)fine_nr, (void)fmt, (void)C, (void)sigma, (void)maxL, (void)theta, (void)omega_s, (void)L_out, (void)mats;
  (void)p_ptr, (void)p_col, (void)p_val, (void)rows, (void)rounds, (void)ms;
  fprintf(stderr, "MG: the aggregation hierarchy is double precision only\n");
  exit(EXIT_FAILURE);
#else
  mg_level* lev    = (mg_level*)calloc((size_t)maxL + 1, sizeof *lev);
  const void* fine = fine_dev;
  CG_UINT n        = fine_nr;
  int L            = 1;
  rows[0]          = n;
  for (int l = 1; l < maxL && n > SBH_MG_SA_COARSEST; l++, L++) {
    mg_level* v  = &lev[l];
    uint32_t nc  = 0;
    sb_csr* p    = sb_matrix_sa_prolongation((const sb_matrix*)fine, theta, omega_s, 0.0, &nc);
    double st[6];
    sb_csr_stats(p, st);
    if (2 * (uint64_t)nc > (uint64_t)n) {
      fprintf(stderr, "MG: aggregation: level %d: %u aggregates of %u rows: the level coarsens by less than 2 (theta = %g)\n", l - 1, nc, n,
          theta);
      exit(EXIT_FAILURE);
    }
    const uint64_t pnnz = sb_csr_nnz(p);
    v->pptr = (uint64_t*)malloc(((size_t)n + 1) * sizeof(uint64_t)), v->pcol = (CG_UINT*)malloc((pnnz + 1) * sizeof(CG_UINT));
    v->pval = (double*)malloc((pnnz + 1) * sizeof(double));
    sb_csr_copy(p, v->pptr, v->pcol, v->pval), sb_csr_free(p);
    sb_csr* ac         = sb_matrix_galerkin((const sb_matrix*)fine, nc, v->pptr, v->pcol, v->pval);
    const uint64_t nnz = sb_csr_nnz(ac);
    uint64_t* ptr      = (uint64_t*)malloc(((size_t)nc + 1) * sizeof(uint64_t));
    CG_UINT* col       = (CG_UINT*)malloc((nnz + 1) * sizeof(CG_UINT));
    double* val        = (double*)malloc((nnz + 1) * sizeof(double));
    double gst[6];
    sb_csr_copy(ac, ptr, col, val), sb_csr_stats(ac, gst), sb_csr_free(ac);
    if (ms) ms[3 * (l - 1)] = st[0], ms[3 * (l - 1) + 1] = st[1] + st[2], ms[3 * (l - 1) + 2] = gst[0] + gst[1];
    rounds[l - 1] = (CG_UINT)st[3], rows[l] = nc;
    sbh_gmatrix_from_csr(&v->gm, nc, ptr, col, val);
    free(ptr), free(col), free(val);
    Comm cc;
    memset(&cc, 0, sizeof cc);
    cc.size = 1;
    commPartition(&cc, &v->gm);
    if (fmt == 0) {
      sbh_convert_crs(&v->crs, &v->gm);
      v->dev = v->crs.dev;
    } else {
      v->scs.C = C, v->scs.sigma = sigma;
      sbh_convert_scs(&v->scs, &v->gm);
      v->dev = v->scs.dev;
    }
    mats[l - 1] = v->dev, p_ptr[l - 1] = v->pptr, p_col[l - 1] = v->pcol, p_val[l - 1] = v->pval;
    fine = v->dev, n = nc;
  }
  *L_out = L;
  return lev;
#endif
}

void sbh_mg_hierarchy_free(void* hierarchy, int fmt, int L)
{
  mg_level* lev = (mg_level*)hierarchy;
  for (int l = 1; l < L; l++) level_free(&lev[l], fmt);
  free(lev);
}
