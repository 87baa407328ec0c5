"""The numerical contract of MG-preconditioned CG restated on the CPU on top of sgs_ref's pieces: a hierarchy of
levels 0 .. L-1, each with sgs_ref's Plan (kept lists, colouring, lower / upper halves) and dinv, an injection map f2c_l between
neighbours, and the apply z = V(0, r).  TEST INFRASTRUCTURE ONLY.

Everything is in each level's DEVICE row order.  Every operation is rounded on its own; double precision, tree dot order.

  V(l, r):
    1  z = sgs_ref's apply on level l (from zero: forward over colours 0 .. nC-1 keeping t, backward over nC-2 .. 0)
    2  if l = L-1: return z
    3  for every coarse row c, f = f2c_l[c]:  s = r_f ;  for every stored entry e of row f of A_l with val_e != 0.0, in storage
       order, the diagonal included:  s = s - a_e * z[col_e] ;  rc_c = s
    4  zc = V(l+1, rc)
    5  z[f2c_l[c]] = z[f2c_l[c]] + zc_c
    6  forward over colours 0 .. nC-1, row i:  s = r_i ; lower(i): s = s - a_e z[col_e] ; t_i = s ; upper(i): s = s - a_e z[col_e] ;
       z_i = s * dinv_i;  backward over nC-2 .. 0, row i:  s = t_i ; upper(i): s = s - a_e z[col_e] ; z_i = s * dinv_i

`solve` is sgs_ref.solve with z = V(0, r).  With L = 1 the hierarchy is sgs_ref's Plan bit for bit.  tests/test_mg_host.py pins
this restatement before anything on the GPU is compared with it.
"""
import math

import numpy as np

from oracle import pyoracle as po

import pcg_ref
import sgs_ref
from sgs_ref import operator, same_bits, unhex, record, csr, gmatrix, problem_args, probe_vector  # noqa: F401  (re-exported)

AUTO_DEPTH = 4  # HPCG's


def geometric_levels(dims, levels=None):
    """L of the geometric hierarchy: `levels`, or None for the deepest L <= 4.  L levels need every dimension divisible by
    2^(L-1) and every coarse dimension >= 2; ValueError says which fails"""
    if levels is not None:
        if levels < 1:
            raise ValueError("levels must be 1 or more")
        f = 2 ** (levels - 1)
        if any(d % f for d in dims):
            raise ValueError("%d levels need every dimension divisible by %d" % (levels, f))
        if levels > 1 and any(d // f < 2 for d in dims):
            raise ValueError("%d levels would give a coarse dimension smaller than 2" % levels)
        return levels
    for L in range(AUTO_DEPTH, 0, -1):
        try:
            return geometric_levels(dims, L)
        except ValueError:
            pass


def geometric_f2c(dims):
    """coarse (x, y, z) of the halved grid -> fine (2x, 2y, 2z), the generator's lexicographic numbering (x fastest)"""
    nx, ny, nz = dims
    if nx % 2 or ny % 2 or nz % 2:
        raise ValueError("odd dimension")
    z, y, x = np.meshgrid(np.arange(nz // 2), np.arange(ny // 2), np.arange(nx // 2), indexing="ij")
    return (((2 * z) * ny + 2 * y) * nx + 2 * x).ravel().astype(np.int64)


def _sub(s, z, ln, cc, vv):
    """s = s - a z[col] down the padded rectangle (len, col, val), entry by entry in storage order; rows side by side"""
    for j in range(cc.shape[1]):
        m = ln > j
        s[m] = s[m] - vv[m, j] * z[cc[m, j]]
    return s


class Level:
    def __init__(self, g, op):
        self.g, self.op, self.n = g, op, g.nr
        self.plan = sgs_ref.Plan(g, op)
        self.dinv = op.to_dev(pcg_ref.jacobi(g))
        self.fine = None  # per coarse device row: the device row of this level it is injected from

    def set_injection(self, f2c, coarse_op):
        """f2c: coarse original row -> this level's original row; translated through both permutations"""
        f2c = np.asarray(f2c, dtype=np.int64)
        assert len(np.unique(f2c)) == len(f2c) and f2c.min() >= 0 and f2c.max() < self.n
        fdev = f2c if self.op.o2n is None else self.op.o2n[f2c]
        self.fine = np.empty(len(f2c), dtype=np.int64)
        self.fine[np.arange(len(f2c)) if coarse_op.o2n is None else coarse_op.o2n] = fdev
        # the stored non-zero entries of the fine rows, the diagonal included, as a padded rectangle in storage order
        ptr, col, val = sgs_ref.device_rows(self.g, self.op)
        lens = np.diff(ptr)[self.fine]
        src = np.repeat(ptr[self.fine], lens) + (np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens))
        which = np.repeat(np.arange(len(self.fine)), lens)
        keep = val[src] != 0.0
        which, c, v = which[keep], col[src][keep], val[src][keep]
        ln = np.bincount(which, minlength=len(self.fine))
        start = np.concatenate(([0], np.cumsum(ln)))
        pos = np.arange(len(which)) - start[which]
        w = int(ln.max()) if len(ln) else 0
        self.rlen, self.rcol, self.rval = ln, np.zeros((len(ln), w), dtype=np.int64), np.zeros((len(ln), w))
        self.rcol[which, pos], self.rval[which, pos] = c, v

    def restrict_residual(self, r, z):
        return _sub(r[self.fine].copy(), z, self.rlen, self.rcol, self.rval)

    def post_smooth(self, r, z):
        """from the guess z (changed in place); returns t"""
        p, t = self.plan, np.zeros(self.n)
        for c in range(p.nC):
            rows = p.rows[c]
            s = _sub(r[rows].copy(), z, *p.half[0][c])
            t[rows] = s
            s = _sub(s, z, *p.half[1][c])
            z[rows] = s * self.dinv[rows]
        for c in range(p.nC - 2, -1, -1):
            rows = p.rows[c]
            z[rows] = _sub(t[rows].copy(), z, *p.half[1][c]) * self.dinv[rows]
        return t


class Hierarchy:
    """levels: [(g, op), ...] from fine to coarse; f2cs: the L - 1 injection maps in original numbering on both sides"""

    def __init__(self, levels, f2cs):
        assert len(f2cs) == len(levels) - 1
        self.lev = [Level(g, op) for g, op in levels]
        for l, f2c in enumerate(f2cs):
            assert self.lev[l + 1].n == len(f2c) < self.lev[l].n
            self.lev[l].set_injection(f2c, self.lev[l + 1].op)
        self.L, self.n, self.nC = len(self.lev), self.lev[0].n, self.lev[0].plan.nC

    def cycle(self, l, r):
        V = self.lev[l]
        z = V.plan.apply(r, V.dinv)[0]
        if l == self.L - 1:
            return z
        rc = V.restrict_residual(r, z)
        zc = self.cycle(l + 1, rc)
        z[V.fine] = z[V.fine] + zc
        V.post_smooth(r, z)
        return z

    def apply(self, r, dinv=None):
        """z = V(0, r) in level 0's device order; the signature of sgs_ref.Plan.apply, so sgs_ref.solve takes a Hierarchy
        (dinv: level 0's, already held)"""
        with np.errstate(all="ignore"):
            return self.cycle(0, np.asarray(r, dtype=np.float64)), None

    def launches(self):
        """launches of one apply: two smoothing applies, the restriction and the prolongation per level but the last; one apply there"""
        a = [2 * V.plan.nC - 1 for V in self.lev]
        return sum(2 * x + 2 for x in a[:-1]) + a[-1]

    def free(self):
        for V in self.lev:
            V.g.free()


class TwoSweeps:
    """the cycle of one level with its coarse levels taken away: the pre-smoothing apply from zero, then the post-smoothing from
    that guess.  What the hierarchy adds is measured against it"""

    def __init__(self, level):
        self.V, self.n, self.nC = level, level.n, level.plan.nC

    def apply(self, r, dinv=None):
        with np.errstate(all="ignore"):
            z = self.V.plan.apply(np.asarray(r, dtype=np.float64), self.V.dinv)[0]
            self.V.post_smooth(r, z)
        return z, None


def solve(op, hier, b_orig, dinv_orig, itermax, eps, keep_x=False):
    return sgs_ref.solve(op, hier, b_orig, dinv_orig, itermax, eps, keep_x)


def dims_of(matrix):
    return (matrix[1],) * 3 if matrix[0] == "hpcg" else tuple(matrix[1:])


def build_hierarchy(c, tmpdir=None):
    """the Hierarchy of a case dict of mg_cases: `levels` (an int, or None for auto) on a generated matrix, or `coarse`: a list
    of (matrix, f2c) with f2c an array or ("geo", nx, ny, nz), the geometric map of that grid"""
    g = gmatrix(c["matrix"], tmpdir)
    levels, f2cs = [(g, operator(g, c["fmt"], c["C"], c["sigma"]))], []
    if c.get("coarse") is not None:
        for matrix, f2c in c["coarse"]:
            gc = gmatrix(matrix, tmpdir)
            levels.append((gc, operator(gc, c["fmt"], c["C"], c["sigma"])))
            f2cs.append(geometric_f2c(f2c[1:]) if isinstance(f2c, tuple) else np.asarray(f2c))
    else:
        dims = dims_of(c["matrix"])
        for _ in range(geometric_levels(dims, c.get("levels")) - 1):
            f2cs.append(geometric_f2c(dims))
            dims = tuple(d // 2 for d in dims)
            gc = po.GMatrix.generate(*dims)
            levels.append((gc, operator(gc, c["fmt"], c["C"], c["sigma"])))
    return Hierarchy(levels, f2cs), f2cs


def build_case(c, tmpdir=None):
    """(hierarchy, f2cs, operator of level 0, b, dinv, eps); b and dinv in original row order"""
    hier, f2cs = build_hierarchy(c, tmpdir)
    g, op = hier.lev[0].g, hier.lev[0].op
    b = g.rhs()
    eps = c["eps_rel"] * math.sqrt(po.ddot_tree(op.to_dev(b), op.to_dev(b)))
    return hier, f2cs, op, b, pcg_ref.jacobi(g), eps


def run_case(c, tmpdir=None):
    hier, f2cs, op, b, dinv, eps = build_case(c, tmpdir)
    out = solve(op, hier, b, dinv, c["itermax"], eps)
    out["eps"], out["dinv"], out["nC"], out["L"] = eps, dinv, [V.plan.nC for V in hier.lev], hier.L
    out["rows"] = [V.n for V in hier.lev]
    hier.free()
    return out
