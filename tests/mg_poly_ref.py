"""The numerical contract of the Chebyshev-smoothed V-cycle restated on the CPU from poly_ref's and mg_fw_ref's
pieces: per level poly_ref's Plan (dinv, the bound, the coefficients, the apply from zero) in the Gauss-Seidel sweeps' place,
between the levels mg_fw_ref's transfers, the restriction reading r and w = A z in the residual's place.  TEST INFRASTRUCTURE ONLY.

Everything is in each level's DEVICE row order.  Every operation is rounded on its own; double precision, tree dot order.

  V(l, r):
    1  z = poly_ref.Plan.apply's steps on level l (from zero), `steps` of them; the last level `coarse_steps`
    2  if l = L-1: return z
    3  w = A_l z
    4  every coarse row c:  s = +0.0 ; the entries of row c of P_l^T with w_e != 0.0 in ascending ORIGINAL fine row number:
       u = r[row_e] - w[row_e] ; s = s + w_e * u ;  rc_c = omega_l * s
    5  zc = V(l+1, rc)
    6  mg_fw_ref's prolongation: z_i = z_i + sum w_e zc[col_e] on the rows with a kept entry
    7  w = A_l z ;  every row: u = r_i - w_i ; u = u * dinv_i ; d_i = u * c1 ; z_i = z_i + d_i ;  then for j = 2 .. steps:
       w = A_l z ; poly_ref.step

A_l z is the level's selected SpMV, and in a Sell-C-sigma format that is more than the oracle's row sums: the format pads every
row to its chunk's longest with (column 0, value 0.0), and the kernels multiply the padding, so a padded row's sum
ends with + 0.0 * z[0] (device row 0).  That changes nothing while z[0] is finite and the sum is not -0.0; a NaN or an inf in z[0]
reaches every padded row.  Inside a cycle the probes' NaN does get there, so `Level.spmv` adds the term (once: adding it again
changes nothing).

`solve` is sgs_ref.solve with z = V(0, r).  With L = 1 the hierarchy is poly_ref's Plan (steps := coarse_steps) bit for bit.
tests/test_mg_poly_host.py pins this restatement before anything on the GPU is compared with it.
"""
import math

import numpy as np

from oracle import pyoracle as po

import mg_fw_ref
import pcg_ref
import poly_ref
import sgs_ref
from mg_fw_ref import trilinear, dims_of, geometric_levels  # noqa: F401  (re-exported)
from sgs_ref import operator, same_bits, unhex, record, csr, gmatrix, problem_args, probe_vector, device_rows  # noqa: F401

OMEGA = 0.25  # with the trilinear P and the stencil regenerated on the coarser grid (DESIGN 4.16's experiment; mgfw keeps 0.5)
STEPS, RATIO = 2, 4.0


class Level(mg_fw_ref.Level):
    """mg_fw_ref's transfers (set_transfer, prolong) around poly_ref's Plan; no colouring"""

    def __init__(self, g, op, steps, lmax, ratio, fmt=("crs", 64, 1)):
        self.g, self.op, self.n, self.fmt = g, op, g.nr, fmt
        self.plan = poly_ref.Plan(g, op, steps, lmax, ratio)
        self.dinv, self.steps = self.plan.dinv, steps
        self.pad = None  # Sell-C-sigma: the device rows shorter than their chunk's longest
        if fmt[0] == "scs":
            lens, C = np.diff(device_rows(g, op)[0]), fmt[1]
            nch = (g.nr + C - 1) // C
            padded = np.zeros(nch * C, dtype=np.int64)
            padded[:g.nr] = lens
            self.pad = (padded.reshape(nch, C) < padded.reshape(nch, C).max(axis=1)[:, None]).ravel()[:g.nr]

    def spmv(self, x):
        """the level's SpMV with the padding's term: + 0.0 * x[0] behind the stored entries of a padded row"""
        w = self.op.spmv(x)
        if self.pad is not None and self.pad.any():
            w[self.pad] = w[self.pad] + np.float64(0.0) * x[0]
        return w

    def smooth(self, r):
        """poly_ref.Plan.apply from zero with this level's SpMV"""
        c = self.plan.c
        d = (r * self.dinv) * np.float64(c["c1"])
        z = d.copy()
        for j in range(2, self.steps + 1):
            d, z = poly_ref.step(r, self.spmv(z), self.dinv, d, z, c["a"][j], c["b"][j])
        return z

    def restrict_diff(self, r, w):
        """step 4: the difference per entry, in registers as it were; no residual vector"""
        ln, cc, vv = self.PT
        s = np.zeros(len(ln))
        for j in range(cc.shape[1]):
            m = ln > j
            u = r[cc[m, j]] - w[cc[m, j]]
            s[m] = s[m] + vv[m, j] * u
        return self.omega * s

    def first(self, r, w, z):
        """step 1 of the post-smoothing behind w = A z: (d, z)"""
        u = r - w
        u = u * self.dinv
        d = u * np.float64(self.plan.c["c1"])
        return d, z + d

    def post_smooth(self, r, z):
        c = self.plan.c
        d, z = self.first(r, self.spmv(z), z)
        for j in range(2, self.steps + 1):
            d, z = poly_ref.step(r, self.spmv(z), self.dinv, d, z, c["a"][j], c["b"][j])
        return z

    def spmv_bytes(self):
        """sb_matrix_spmv_bytes of this level's matrix in the operator's format"""
        g, op = self.g, self.op
        if self.fmt[0] == "crs":
            return 12.0 * int(g.rowPtr[g.nr]) + 4.0 * (g.nr + 1) + 8.0 * g.nr + 8.0 * g.nc
        C = self.fmt[1]
        lens = np.diff(device_rows(g, op)[0])
        nch = (g.nr + C - 1) // C
        padded = np.zeros(nch * C, dtype=np.int64)
        padded[:g.nr] = lens
        n_elems = int(padded.reshape(nch, C).max(axis=1).sum()) * C
        return 12.0 * n_elems + 8.0 * nch + 8.0 * nch * C + 8.0 * g.nc

    def transfer_bytes(self):
        """both Sell-64 structures as one cycle reads them: 12 B per padded element, 64 row lengths and 12 B per chunk"""
        b = 0.0
        for ln in (self.PT[0], self.P[0]):
            nch = (len(ln) + 63) // 64
            padded = np.zeros(nch * 64, dtype=np.int64)
            padded[:len(ln)] = ln
            b += 12.0 * int(padded.reshape(nch, 64).max(axis=1).sum()) * 64 + nch * (64.0 * 4 + 12.0)
        return b


class Hierarchy:
    """levels: [(g, op), ...] from fine to coarse; ps: the L - 1 prolongations (ptr, col, val); omegas: their restrictions' scales;
    fmt: (format, C, sigma) the operators were made with, for the byte model alone"""

    def __init__(self, levels, ps, omegas, steps=STEPS, coarse_steps=None, lmax=None, ratio=RATIO, fmt=("crs", 64, 1)):
        assert len(ps) == len(omegas) == len(levels) - 1
        coarse_steps = steps if coarse_steps is None else coarse_steps
        L = len(levels)
        self.lev = [Level(g, op, coarse_steps if l == L - 1 else steps, lmax, ratio, fmt) for l, (g, op) in enumerate(levels)]
        for l, (P, omega) in enumerate(zip(ps, omegas)):
            assert self.lev[l + 1].n < self.lev[l].n
            self.lev[l].set_transfer(P, omega, self.lev[l + 1].op, self.lev[l + 1].n)
        self.L, self.n, self.steps, self.coarse_steps = L, self.lev[0].n, steps, coarse_steps
        self.dinv = self.lev[0].dinv

    def cycle(self, l, r):
        V = self.lev[l]
        z = V.smooth(r)
        if l == self.L - 1:
            return z
        rc = V.restrict_diff(r, V.spmv(z))
        zc = self.cycle(l + 1, rc)
        V.prolong(z, zc)
        return V.post_smooth(r, z)

    def apply(self, r, dinv=None):
        """z = V(0, r) in level 0's device order; the signature of sgs_ref.Plan.apply"""
        with np.errstate(all="ignore"):
            return self.cycle(0, np.asarray(r, dtype=np.float64)), None

    def probe(self, l, r, w, z, zc):
        """steps 4 and 6 on level l alone, device order: (rc, z after prolonging zc)"""
        V = self.lev[l]
        with np.errstate(all="ignore"):
            return V.restrict_diff(np.asarray(r, dtype=np.float64), np.asarray(w, dtype=np.float64)), \
                V.prolong(np.array(z, dtype=np.float64), zc)

    def launches(self):
        """of one cycle, level 0's step 1 (in the r update) among them: per level but the last 2 steps - 1 for the pre-smoothing,
        the SpMV of step 3, the restriction, the prolongation, 2 steps for the post-smoothing; the last level 2 coarse_steps - 1"""
        return sum((2 * V.steps - 1) + 1 + 1 + 1 + 2 * V.steps for V in self.lev[:-1]) + 2 * self.lev[-1].steps - 1

    def launches_per_body(self, fused_dot=True):
        """p update | SpMV (+ dot pass) | alpha | the cycle | beta"""
        return (4 if fused_dot else 5) + self.launches()

    def bytes(self):
        """the byte model of one cycle, counted operation by operation"""
        b = 0.0
        for V in self.lev:
            n, last = float(V.n), V is self.lev[-1]
            b += 24.0 * n  # step 1: r, dinv in; d, z out (d = z: counted as the polynomial handle counts it)
            b += (V.steps - 1) * (V.spmv_bytes() + 56.0 * n)  # steps 2 .. of the pre-smoothing
            if last:
                break
            b += V.spmv_bytes()  # w = A z
            b += V.transfer_bytes() + 2 * 8.0 * n + 8.0 * V.nc  # P^T: r and w gathered, rc out
            b += 8.0 * V.nc + 16.0 * n  # P: zc gathered, z in and out
            b += V.spmv_bytes() + 48.0 * n  # the post-smoothing's step 1
            b += (V.steps - 1) * (V.spmv_bytes() + 56.0 * n)
        return b

    def free(self):
        for V in self.lev:
            V.g.free()


def solve(op, hier, b_orig, itermax, eps, keep_x=False):
    return sgs_ref.solve(op, hier, b_orig, op.to_orig(hier.dinv), itermax, eps, keep_x)


def galerkin_gmatrix(A, P):
    """(GMatrix, scipy CSR) of P^T A P with sorted columns and exact zeros dropped"""
    Ac = (P.T.tocsr() @ A @ P).tocsr()
    Ac.sum_duplicates()
    Ac.eliminate_zeros()
    Ac.sort_indices()
    g = po.GMatrix.from_csr(Ac.indptr.astype(np.uint32), Ac.indices.astype(np.uint32), Ac.data.astype(np.float64), nc=Ac.shape[1])
    return g, Ac


def case_transfers(c):
    """the (P, omega) list of a case dict, original numbering: mg_fw_ref's with omega = 0.25 on the regenerated hierarchy and 1.0
    on the Galerkin one"""
    if c.get("coarse") is not None:
        return [(trilinear(P[1:]) if isinstance(P[0], str) else P, omega) for _, P, omega in c["coarse"]]
    dims, out = dims_of(c["matrix"]), []
    for _ in range(geometric_levels(dims, c.get("levels")) - 1):
        out.append((trilinear(dims), 1.0 if c.get("galerkin") else OMEGA))
        dims = tuple(d // 2 for d in dims)
    return out


def build_hierarchy(c, tmpdir=None):
    """the Hierarchy of a case dict of mg_poly_cases: `levels` on a generated matrix (galerkin: A_{l+1} = P_l^T A_l P_l in the
    regenerated stencil's place) or `coarse`: [(matrix, P, omega), ...]; `steps`, `coarse_steps`, `lmax`, `ratio` optional"""
    g = gmatrix(c["matrix"], tmpdir)
    fmt = (c["fmt"], c["C"], c["sigma"])
    levels = [(g, operator(g, *fmt))]
    transfers = case_transfers(c)
    if c.get("coarse") is not None:
        gs = [gmatrix(m, tmpdir) for m, _, _ in c["coarse"]]
    elif c.get("galerkin"):
        import scipy.sparse as sp
        A, gs = csr(g), []
        for (ptr, col, val), _ in transfers:
            P = sp.csr_matrix((val, col, ptr), shape=(A.shape[0], A.shape[0] // 8))
            gc, A = galerkin_gmatrix(A, P)
            gs.append(gc)
    else:
        dims, gs = dims_of(c["matrix"]), []
        for _ in transfers:
            dims = tuple(d // 2 for d in dims)
            gs.append(gmatrix(("dims",) + dims, tmpdir))
    levels += [(gc, operator(gc, *fmt)) for gc in gs]
    hier = Hierarchy(levels, [P for P, _ in transfers], [w for _, w in transfers], c.get("steps", STEPS), c.get("coarse_steps"),
                     c.get("lmax"), c.get("ratio", RATIO), fmt)
    return hier, transfers


def build_case(c, tmpdir=None):
    """(hierarchy, transfers, operator of level 0, b, eps); b in original row order"""
    hier, transfers = build_hierarchy(c, tmpdir)
    g, op = hier.lev[0].g, hier.lev[0].op
    b = g.rhs()
    eps = c["eps_rel"] * math.sqrt(po.ddot_tree(op.to_dev(b), op.to_dev(b)))
    return hier, transfers, op, b, eps


def run_case(c, tmpdir=None):
    hier, transfers, op, b, eps = build_case(c, tmpdir)
    out = solve(op, hier, b, c["itermax"], eps)
    out["eps"], out["dinv"], out["L"], out["rows"] = eps, op.to_orig(hier.dinv), hier.L, [V.n for V in hier.lev]
    out["coeffs"] = [poly_ref.coeff_array(V.plan.c) for V in hier.lev]
    out["intervals"] = [(V.plan.c["lmin"], V.plan.c["lmax"]) for V in hier.lev]
    out["launches"], out["bytes"] = hier.launches_per_body(), hier.bytes()
    hier.free()
    return out


def count_table(n):
    """k to eps = 1e-10 ||b|| on the n^3 stencil in CRS order at the deepest hierarchy, ratio 4: Jacobi, the polynomial (3, 16), and
    for steps 1, 2, 3 the regenerated hierarchy at omega = 0.5 and 0.25 and the Galerkin one (DESIGN 4.16's table)"""
    base = dict(matrix=("hpcg", n), fmt="crs", C=64, sigma=1, itermax=300, eps_rel=1e-10)
    g, op, b, dinv, eps = pcg_ref.build_case(dict(base, dinv="jacobi"))
    row = {"jacobi": int(pcg_ref.solve(op, b, dinv, 300, eps)["k"]),
           "poly_3_16": int(poly_ref.solve(op, poly_ref.Plan(g, op, 3, None, 16.0), b, 300, eps)["k"])}
    g.free()
    L = geometric_levels((n, n, n), None)
    half, dims = [], (n, n, n)
    for _ in range(L - 1):  # the regenerated hierarchy spelled out, to carry omega = 0.5
        half.append((("dims",) + tuple(d // 2 for d in dims), ("tri",) + dims, 0.5))
        dims = tuple(d // 2 for d in dims)
    for name, kw in (("regenerated_omega_0.5", dict(coarse=half)), ("regenerated_omega_0.25", dict(levels=None)),
                     ("galerkin", dict(levels=None, galerkin=True))):
        row[name] = []
        for steps in (1, 2, 3):
            hier, transfers, op, b, eps = build_case(dict(base, steps=steps, **kw))
            row[name].append(int(solve(op, hier, b, 300, eps)["k"]))
            hier.free()
    return row


def dense_apply(hier):
    """the matrix of the cycle, column by column (small n)"""
    n = hier.n
    M = np.zeros((n, n))
    for i in range(n):
        e = np.zeros(n)
        e[i] = 1.0
        M[:, i] = hier.apply(e)[0]
    return M
