"""The numerical contract of SGS-preconditioned CG restated on the CPU: kept lists, the symmetrised greedy
colouring, the lower / upper split, the apply z = M^-1 r with M = (D + L) D^-1 (D + U) in the colour order, and `solve` --
pcg_ref.solve with `z = r * dinv` replaced by the apply -- on top of pcg_ref's pieces.  TEST INFRASTRUCTURE ONLY.

Everything is in the DEVICE's row order (`op.to_dev`).  Every operation is rounded on its own: s = s - a * z[col] is one numpy
multiply and one subtraction per entry, rows of a colour side by side (they do not couple), entries of a row in storage order.
tests/test_sgs_host.py pins this restatement before anything on the GPU is compared with it.
"""
import math

import numpy as np

from oracle import pyoracle as po

import pcg_ref
from pcg_ref import operator, same_bits, unhex, record, csr, gmatrix, problem_args  # noqa: F401  (re-exported for the tests)


def device_rows(g, op):
    """(ptr, col, val) of the matrix in the device's numbering: device row d holds original row n2o[d]'s stored entries in
    storage order, columns renumbered"""
    rp, col, val = g.rowPtr.astype(np.int64), g.col.astype(np.int64), g.val
    n = g.nr
    rows = np.arange(n) if op.o2n is None else op.n2o
    lens = np.diff(rp)[rows]
    ptr = np.concatenate(([0], np.cumsum(lens)))
    src = np.repeat(rp[rows] - ptr[:-1], lens) + np.arange(ptr[-1])
    c = col[src]
    return ptr, (c if op.o2n is None else op.o2n[c]), val[src].copy()


def kept(ptr, col, val):
    """the kept entries: stored, off the diagonal, non-zero; storage order"""
    n = len(ptr) - 1
    row = np.repeat(np.arange(n), np.diff(ptr))
    keep = (col != row) & (val != 0.0)
    kptr = np.concatenate(([0], np.cumsum(np.bincount(row[keep], minlength=n))))
    return kptr, col[keep], val[keep]


def colouring(kptr, kcol):
    """rows 0, 1, ... each take the smallest colour no adjacent, already coloured row has; adjacent: a_ij or a_ji kept"""
    n = len(kptr) - 1
    row = np.repeat(np.arange(n), np.diff(kptr))
    order = np.argsort(kcol, kind="stable")
    tptr = np.concatenate(([0], np.cumsum(np.bincount(kcol, minlength=n))))
    trow = row[order]
    colour = np.zeros(n, dtype=np.int64)
    kc, tr, kp, tp = kcol.tolist(), trow.tolist(), kptr.tolist(), tptr.tolist()
    col_l = [0] * n
    for i in range(n):
        taken = {col_l[j] for j in kc[kp[i]:kp[i + 1]] if j < i}
        taken.update(col_l[j] for j in tr[tp[i]:tp[i + 1]] if j < i)
        c = 0
        while c in taken:
            c += 1
        col_l[i] = c
    colour[:] = col_l
    return colour


class Plan:
    """colour, nC, and per colour the rows (ascending) with their lower and upper entries padded to rectangles"""

    def __init__(self, g, op):
        ptr, col, val = device_rows(g, op)
        self.n = g.nr
        self.kptr, self.kcol, self.kval = kept(ptr, col, val)
        self.colour = colouring(self.kptr, self.kcol)
        self.nC = int(self.colour.max()) + 1 if self.n else 0
        row = np.repeat(np.arange(self.n), np.diff(self.kptr))
        ci, cj = self.colour[row], self.colour[self.kcol]
        assert not np.any(ci == cj), "adjacent rows share a colour"
        self.rows = [np.nonzero(self.colour == c)[0] for c in range(self.nC)]
        self.half = [self._rect(row, cj < ci), self._rect(row, cj > ci)]

    def _rect(self, row, sel):
        """per colour: (len, col[rows, maxlen], val[rows, maxlen]) of the selected entries, storage order kept"""
        r, c, v = row[sel], self.kcol[sel], self.kval[sel]
        lens = np.bincount(r, minlength=self.n)
        ptr = np.concatenate(([0], np.cumsum(lens)))
        pos = np.arange(len(r)) - ptr[r]  # r is ascending: position of the entry within its row
        out = []
        for rows in self.rows:
            ln = lens[rows]
            w = int(ln.max()) if len(rows) else 0
            cc, vv = np.zeros((len(rows), w), dtype=np.int64), np.zeros((len(rows), w))
            where = np.full(self.n, -1, dtype=np.int64)
            where[rows] = np.arange(len(rows))
            m = where[r] >= 0
            cc[where[r[m]], pos[m]], vv[where[r[m]], pos[m]] = c[m], v[m]
            out.append((ln, cc, vv))
        return out

    def lower(self, i):
        return self._entries(i, 0)

    def upper(self, i):
        return self._entries(i, 1)

    def _entries(self, i, h):
        c = self.colour[i]
        k = int(np.searchsorted(self.rows[c], i))
        ln, cc, vv = self.half[h][c]
        return cc[k, :ln[k]], vv[k, :ln[k]]

    def apply(self, r, dinv):
        """z (device order) of r and dinv (device order); also returns t"""
        z, t = np.zeros(self.n), np.zeros(self.n)
        with np.errstate(all="ignore"):
            for c in range(self.nC):
                s = self._sweep(r, z, c, 0)
                t[self.rows[c]] = s
                z[self.rows[c]] = s * dinv[self.rows[c]]
            for c in range(self.nC - 2, -1, -1):
                s = self._sweep(t, z, c, 1)
                z[self.rows[c]] = s * dinv[self.rows[c]]
        return z, t

    def _sweep(self, src, z, c, h):
        ln, cc, vv = self.half[h][c]
        s = src[self.rows[c]].copy()
        for j in range(cc.shape[1]):
            m = ln > j
            s[m] = s[m] - vv[m, j] * z[cc[m, j]]
        return s


def apply_scalar(plan, r, dinv):
    """the apply entry by entry, as the contract words it (small matrices: pins the vectorised apply above)"""
    n = plan.n
    z, t = np.zeros(n), np.zeros(n)
    with np.errstate(all="ignore"):
        for c in range(plan.nC):
            for i in plan.rows[c]:
                s = np.float64(r[i])
                for col, a in zip(*plan.lower(i)):
                    s = s - a * z[col]
                t[i] = s
                z[i] = s * dinv[i]
        for c in range(plan.nC - 2, -1, -1):
            for i in plan.rows[c]:
                s = np.float64(t[i])
                for col, a in zip(*plan.upper(i)):
                    s = s - a * z[col]
                z[i] = s * dinv[i]
    return z


def solve(op, plan, b_orig, dinv_orig, itermax, eps, keep_x=False):
    """pcg_ref.solve with z = r * dinv replaced by the apply: k, rr, rz, pAp, x (original row order); keep_x: also `xs`, the
    iterate after every body"""
    b = op.to_dev(np.asarray(b_orig, dtype=np.float64))
    dinv = op.to_dev(np.asarray(dinv_orig, dtype=np.float64))
    n = len(b)
    x = np.zeros(n)
    rr, rz, pAp, xs = [], [], [], []
    with np.errstate(all="ignore"):
        p = po.waxpby(1.0, x, 0.0, x)
        Ap = op.spmv(p)
        r = po.waxpby(1.0, b, -1.0, Ap)
        z = plan.apply(r, dinv)[0]
        rtrans = np.float64(po.ddot_tree(r, r))
        rztrans = np.float64(po.ddot_tree(r, z))
        rr.append(rtrans), rz.append(rztrans)
        normr = np.sqrt(rtrans)
        k = 1
        while k < itermax and normr > eps:
            if k == 1:
                p = po.waxpby(1.0, z, 0.0, z)
            else:
                oldrz = rztrans
                z = plan.apply(r, dinv)[0]
                rztrans = np.float64(po.ddot_tree(r, z))
                rtrans = np.float64(po.ddot_tree(r, r))
                rr.append(rtrans), rz.append(rztrans)
                beta = rztrans / oldrz
                p = po.waxpby(1.0, z, float(beta), p)
            normr = np.sqrt(rtrans)
            Ap = op.spmv(p)
            alpha = np.float64(po.ddot_tree(p, Ap))
            pAp.append(alpha)
            alpha = rztrans / alpha
            x = po.waxpby(1.0, x, float(alpha), p)
            if keep_x:
                xs.append(op.to_orig(x))
            r = po.waxpby(1.0, r, float(-alpha), Ap)
            k += 1
    f = lambda a: np.array(a, dtype=np.float64)  # noqa: E731
    return dict(k=k, rr=f(rr), rz=f(rz), pAp=f(pAp), x=op.to_orig(x), xs=xs)


def build_case(c, tmpdir=None):
    """(g, operator, plan, b, dinv, eps) of a case dict of sgs_cases; b and dinv in original row order"""
    g = gmatrix(c["matrix"], tmpdir)
    op = operator(g, c["fmt"], c["C"], c["sigma"])
    b = g.rhs()
    eps = c["eps_rel"] * math.sqrt(po.ddot_tree(op.to_dev(b), op.to_dev(b)))
    return g, op, Plan(g, op), b, pcg_ref.jacobi(g), eps


def run_case(c, tmpdir=None):
    g, op, plan, b, dinv, eps = build_case(c, tmpdir)
    out = solve(op, plan, b, dinv, c["itermax"], eps)
    out["eps"], out["dinv"], out["nC"] = eps, dinv, plan.nC
    g.free()
    return out


def probe_vector(n, seed, special=False):
    """an r of mixed sign and magnitude holding +0.0, -0.0 and a denormal; special: an inf and a NaN as well"""
    rng = np.random.RandomState(seed)
    r = rng.standard_normal(n) * 10.0 ** rng.randint(-8, 9, size=n)
    r[0 % n] = 0.0
    if n > 1:
        r[n // 2] = -0.0
    if n > 2:
        r[n - 1] = 5e-324 * 1000
    if n > 3:
        r[1] = -0.0
    if special and n > 5:
        r[n // 3] = np.inf
        r[(2 * n) // 3] = np.nan
    return r
