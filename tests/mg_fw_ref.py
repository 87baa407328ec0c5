"""The numerical contract of the V-cycle with full-weighting transfers restated on the CPU on top of mg_ref's and
sgs_ref's pieces: the levels, their Plans and the post-smoothing are mg_ref's; between them a prolongation P_l (CSR, n_l x
n_{l+1}, original numbering on both sides) and the restriction omega_l P_l^T of the FULL residual.  TEST INFRASTRUCTURE ONLY.

Everything is in each level's DEVICE row order.  Every operation is rounded on its own; double precision, tree dot order.

  V(l, r):
    1  z = sgs_ref's apply on level l (from zero)
    2  if l = L-1: return z
    3  every row i:  s = r_i ; lower(i) in storage order: s = s - a_e z[col_e] ; upper(i) likewise ; s = s - diag_i * z_i ; d_i = s
    4  every coarse row c:  s = +0.0 ; the entries of row c of P_l^T with w_e != 0.0 in ascending ORIGINAL fine row number:
       s = s + w_e * d[row_e] ;  rc_c = omega_l * s
    5  zc = V(l+1, rc)
    6  every fine row i with a kept entry in P_l:  s = +0.0 ; its entries with w_e != 0.0 in storage order: s = s + w_e * zc[col_e] ;
       z_i = z_i + s   (other rows untouched)
    7  mg_ref's post-smoothing from the guess

`solve` is sgs_ref.solve with z = V(0, r).  With L = 1 the hierarchy is sgs_ref's Plan bit for bit.  tests/test_mg_fw_host.py pins
this restatement before anything on the GPU is compared with it.
"""
import math

import numpy as np

from oracle import pyoracle as po

import mg_ref
import pcg_ref
import sgs_ref
from mg_ref import TwoSweeps, dims_of, geometric_levels  # noqa: F401  (re-exported)
from sgs_ref import operator, same_bits, unhex, record, csr, gmatrix, problem_args, probe_vector  # noqa: F401  (re-exported)

OMEGA = 0.5  # with the trilinear P: P^T A_h P ~ 2 A_H for the unscaled stencil regenerated on the coarser grid


def trilinear(dims):
    """(ptr, col, val) of the trilinear prolongation onto an nx x ny x nz grid (all even) from the halved one, x fastest: per
    dimension an even index i takes coarse i / 2 with weight 1, an odd one (i - 1) / 2 and (i + 1) / 2 with 1/2 each, the second
    dropped where it equals the coarse dimension; a row's entries in ascending coarse number"""
    nx, ny, nz = dims
    if nx % 2 or ny % 2 or nz % 2:
        raise ValueError("odd dimension")
    cx, cy = nx // 2, ny // 2

    def line(i, nc):
        if i % 2 == 0:
            return [(i // 2, 1.0)]
        return [(j, 0.5) for j in ((i - 1) // 2, (i + 1) // 2) if j < nc]

    ptr, col, val = [0], [], []
    for z in range(nz):
        lz = line(z, nz // 2)
        for y in range(ny):
            ly = line(y, cy)
            for x in range(nx):
                for kz, wz in lz:
                    for ky, wy in ly:
                        for kx, wx in line(x, cx):
                            col.append((kz * cy + ky) * cx + kx)
                            val.append(wz * wy * wx)
                ptr.append(len(col))
    return np.array(ptr, dtype=np.int64), np.array(col, dtype=np.int64), np.array(val)


def _rect(row, col, val, n):
    """(len, col[n, w], val[n, w]) of entries already grouped by ascending `row`, their order within a row kept"""
    ln = np.bincount(row, minlength=n)
    start = np.concatenate(([0], np.cumsum(ln)))
    pos = np.arange(len(row)) - start[row]
    w = int(ln.max()) if len(ln) else 0
    cc, vv = np.zeros((n, w), dtype=np.int64), np.zeros((n, w))
    cc[row, pos], vv[row, pos] = col, val
    return ln, cc, vv


def _add(v, ln, cc, vv):
    """s = +0.0 ; s = s + w v[col] down the padded rectangle, entry by entry; rows side by side"""
    s = np.zeros(len(ln))
    for j in range(cc.shape[1]):
        m = ln > j
        s[m] = s[m] + vv[m, j] * v[cc[m, j]]
    return s


class Level(mg_ref.Level):
    def __init__(self, g, op):
        mg_ref.Level.__init__(self, g, op)
        self.diag = op.to_dev(pcg_ref.diagonal(g))

    def set_transfer(self, P, omega, coarse_op, nc):
        """P: (ptr, col, val) in original numbering on both sides; translated through both permutations"""
        ptr, col, val = (np.asarray(a) for a in P)
        ptr, col, val = ptr.astype(np.int64), col.astype(np.int64), val.astype(np.float64)
        assert len(ptr) == self.n + 1 and np.all(np.diff(ptr) >= 0) and (len(col) == 0 or (col.min() >= 0 and col.max() < nc))
        assert np.isfinite(val).all() and np.isfinite(omega) and omega > 0.0
        row = np.repeat(np.arange(self.n), np.diff(ptr))  # ascending original fine row, storage order within
        keep = val != 0.0
        row, col, val = row[keep], col[keep], val[keep]
        fdev = row if self.op.o2n is None else self.op.o2n[row]
        cdev = col if coarse_op.o2n is None else coarse_op.o2n[col]
        o = np.argsort(fdev, kind="stable")  # P: a row's entries in storage order
        self.P = _rect(fdev[o], cdev[o], val[o], self.n)
        o = np.argsort(cdev, kind="stable")  # P^T: a coarse row's entries in ascending original fine row
        self.PT = _rect(cdev[o], fdev[o], val[o], nc)
        self.omega, self.nc = float(omega), nc

    def residual(self, r, z):
        p, d = self.plan, np.zeros(self.n)
        for c in range(p.nC):
            rows = p.rows[c]
            s = mg_ref._sub(r[rows].copy(), z, *p.half[0][c])
            s = mg_ref._sub(s, z, *p.half[1][c])
            d[rows] = s - self.diag[rows] * z[rows]
        return d

    def restrict(self, d):
        return self.omega * _add(d, *self.PT)

    def prolong(self, z, zc):
        """z changed in place: only the rows with a kept entry"""
        s, m = _add(zc, *self.P), self.P[0] > 0
        z[m] = z[m] + s[m]
        return z


class Hierarchy:
    """levels: [(g, op), ...] from fine to coarse; ps: the L - 1 prolongations (ptr, col, val); omegas: their restrictions' scales"""

    def __init__(self, levels, ps, omegas):
        assert len(ps) == len(omegas) == len(levels) - 1
        self.lev = [Level(g, op) for g, op in levels]
        for l, (P, omega) in enumerate(zip(ps, omegas)):
            assert self.lev[l + 1].n < self.lev[l].n
            self.lev[l].set_transfer(P, omega, self.lev[l + 1].op, self.lev[l + 1].n)
        self.L, self.n, self.nC = len(self.lev), self.lev[0].n, self.lev[0].plan.nC

    def cycle(self, l, r):
        V = self.lev[l]
        z = V.plan.apply(r, V.dinv)[0]
        if l == self.L - 1:
            return z
        rc = V.restrict(V.residual(r, z))
        zc = self.cycle(l + 1, rc)
        V.prolong(z, zc)
        V.post_smooth(r, z)
        return z

    def apply(self, r, dinv=None):
        """z = V(0, r) in level 0's device order; the signature of sgs_ref.Plan.apply"""
        with np.errstate(all="ignore"):
            return self.cycle(0, np.asarray(r, dtype=np.float64)), None

    def probe(self, l, r, z, zc):
        """steps 3, 4 and 6 on level l alone, device order: (d, rc, z after prolonging zc)"""
        V = self.lev[l]
        with np.errstate(all="ignore"):
            d = V.residual(np.asarray(r, dtype=np.float64), z)
            return d, V.restrict(d), V.prolong(np.array(z, dtype=np.float64), zc)

    def launches(self):
        """mg_ref's count plus the residual's launch per level but the last"""
        a = [2 * V.plan.nC - 1 for V in self.lev]
        return sum(2 * x + 3 for x in a[:-1]) + a[-1]

    def free(self):
        for V in self.lev:
            V.g.free()


def solve(op, hier, b_orig, dinv_orig, itermax, eps, keep_x=False):
    return sgs_ref.solve(op, hier, b_orig, dinv_orig, itermax, eps, keep_x)


def case_transfers(c):
    """the (P, omega) list of a case dict as the C API and hostapi take it, original numbering; P ("tri", nx, ny, nz) is the
    trilinear one of that grid"""
    if c.get("coarse") is not None:
        return [(trilinear(P[1:]) if isinstance(P[0], str) else P, omega) for _, P, omega in c["coarse"]]
    dims, out = dims_of(c["matrix"]), []
    for _ in range(geometric_levels(dims, c.get("levels")) - 1):
        out.append((trilinear(dims), OMEGA))
        dims = tuple(d // 2 for d in dims)
    return out


def build_hierarchy(c, tmpdir=None):
    """the Hierarchy of a case dict of mg_fw_cases: `levels` (an int, or None for auto) on a generated matrix -- the trilinear P
    and omega = 0.5 -- or `coarse`: a list of (matrix, P, omega)"""
    g = gmatrix(c["matrix"], tmpdir)
    levels = [(g, operator(g, c["fmt"], c["C"], c["sigma"]))]
    transfers = case_transfers(c)
    if c.get("coarse") is not None:
        mats = [m for m, _, _ in c["coarse"]]
    else:
        dims, mats = dims_of(c["matrix"]), []
        for _ in transfers:
            dims = tuple(d // 2 for d in dims)
            mats.append(("dims",) + dims)
    for m in mats:
        gc = gmatrix(m, tmpdir)
        levels.append((gc, operator(gc, c["fmt"], c["C"], c["sigma"])))
    return Hierarchy(levels, [P for P, _ in transfers], [w for _, w in transfers]), transfers


def build_case(c, tmpdir=None):
    """(hierarchy, transfers, operator of level 0, b, dinv, eps); b and dinv in original row order"""
    hier, transfers = build_hierarchy(c, tmpdir)
    g, op = hier.lev[0].g, hier.lev[0].op
    b = g.rhs()
    eps = c["eps_rel"] * math.sqrt(po.ddot_tree(op.to_dev(b), op.to_dev(b)))
    return hier, transfers, op, b, pcg_ref.jacobi(g), eps


def run_case(c, tmpdir=None):
    hier, transfers, op, b, dinv, eps = build_case(c, tmpdir)
    out = solve(op, hier, b, dinv, c["itermax"], eps)
    out["eps"], out["dinv"], out["nC"], out["L"] = eps, dinv, [V.plan.nC for V in hier.lev], hier.L
    out["rows"] = [V.n for V in hier.lev]
    hier.free()
    return out
