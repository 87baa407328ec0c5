"""The numerical contract of restarted GMRES(m) restated on the CPU, on top of the oracle's operations:
`GMatrix.spmv`, `waxpby`, `ddot_tree`.  Classical Gram-Schmidt with one reorthogonalisation, Givens rotations and back
substitution as explicit loops on Python floats (IEEE doubles, every operation rounded on its own); the vector updates as
numpy elementwise operations (product rounded, then the add or subtract).  TEST INFRASTRUCTURE ONLY: lives in tests/, the
product never imports the oracle.

Vectors live in the DEVICE's row order: for a Sell-C-sigma matrix with sigma > 1 that is the permuted order
(v_dev[new] = v_orig[old], `Scs.oldToNewPerm`), which is the order the tree dot walks.
"""
import hashlib
import math
import os
import tempfile

import numpy as np

from oracle import pyoracle as po

import gmres_cases


class Operator:
    """A x in the device's row order; perm = oldToNewPerm (None: the original order)"""

    def __init__(self, g, old_to_new=None):
        self.g = g
        self.o2n = None if old_to_new is None else np.asarray(old_to_new, dtype=np.int64)
        if self.o2n is not None and np.array_equal(self.o2n, np.arange(len(self.o2n))):
            self.o2n = None
        if self.o2n is not None:
            self.n2o = np.empty_like(self.o2n)
            self.n2o[self.o2n] = np.arange(len(self.o2n))

    def to_dev(self, v):
        return np.ascontiguousarray(v if self.o2n is None else v[self.n2o])

    def to_orig(self, v):
        return np.ascontiguousarray(v if self.o2n is None else v[self.o2n])

    def spmv(self, x_dev):
        return self.to_dev(self.g.spmv(self.to_orig(x_dev)))


def multidot(V, w):
    """h[i] = tree dot of V[i] and w (the loop sb_multidot restates)"""
    w = np.ascontiguousarray(w)
    return [po.ddot_tree(np.ascontiguousarray(v), w) for v in V]


def multiaxpy_sub(V, h, w):
    """w[e] = (..((w[e] - h[0]*V[0][e]) - h[1]*V[1][e]) ..), ascending i (the loop sb_multiaxpy_sub restates)"""
    w = np.array(w, dtype=np.float64)
    with np.errstate(all="ignore"):
        for v, hi in zip(V, h):
            w = w - np.float64(hi) * v
    return w


def solve(op, b_dev, m, itermax, eps):
    """The pseudocode of DESIGN 4.8, line for line.  Returns k, res_hist, rr_hist, x (device order) and, per cycle close,
    (estimate, sqrt(rr_true)) in `closes`."""
    n = len(b_dev)
    x = np.zeros(n)
    r = po.waxpby(1.0, b_dev, -1.0, op.spmv(x))
    rr = po.ddot_tree(r, r)
    normr = math.sqrt(rr)
    rr_hist, res_hist, closes = [rr], [normr], []
    V = [None] * (m + 1)
    H = [[0.0] * m for _ in range(m + 1)]
    cs, sn, g = [0.0] * m, [0.0] * m, [0.0] * (m + 1)
    k, j = 1, 0
    with np.errstate(all="ignore"):
        while k < itermax and normr > eps:
            if j == 0:
                V[0] = r / np.float64(normr)
                g[0] = normr
            w = op.spmv(V[j])
            h1 = multidot(V[:j + 1], w)
            w = multiaxpy_sub(V[:j + 1], h1, w)
            h2 = multidot(V[:j + 1], w)
            w = multiaxpy_sub(V[:j + 1], h2, w)
            for i in range(j + 1):
                H[i][j] = h1[i] + h2[i]
            hn = math.sqrt(po.ddot_tree(w, w))
            for i in range(j):
                t = cs[i] * H[i][j] + sn[i] * H[i + 1][j]
                H[i + 1][j] = cs[i] * H[i + 1][j] - sn[i] * H[i][j]
                H[i][j] = t
            d = _sqrt(H[j][j] * H[j][j] + hn * hn)
            cs[j] = _div(H[j][j], d)
            sn[j] = _div(hn, d)
            H[j][j] = d
            g[j + 1] = -(sn[j] * g[j])
            g[j] = cs[j] * g[j]
            normr = abs(g[j + 1])
            res_hist.append(normr)
            k += 1
            j += 1
            go = k < itermax and normr > eps
            if j == m or not go:
                y = [0.0] * j
                for i in range(j - 1, -1, -1):
                    t = g[i]
                    for l in range(i + 1, j):
                        t = t - H[i][l] * y[l]
                    y[i] = _div(t, H[i][i])
                for i in range(j):
                    x = x + np.float64(y[i]) * V[i]
                r = po.waxpby(1.0, b_dev, -1.0, op.spmv(x))
                rr = po.ddot_tree(r, r)
                rr_hist.append(rr)
                closes.append((normr, _sqrt(rr)))
                if not go:
                    break
                normr = _sqrt(rr)
                j = 0
            else:
                V[j] = w / np.float64(hn)
    return dict(k=k, res=np.array(res_hist), rr=np.array(rr_hist), x=x, closes=closes)


def _sqrt(v):
    return float(np.sqrt(np.float64(v)))  # (NaN in, NaN out: no exception)


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def build_case(name, tmpdir=None):
    """(operator, b in device order, m, itermax, eps, g) of a case of gmres_cases.CASES"""
    c = gmres_cases.CASES[name]
    if c["kind"] == "cd":
        tmpdir = tmpdir or tempfile.mkdtemp(prefix="gmres_cd_")
        path = gmres_cases.write_convdiff(os.path.join(str(tmpdir), "cd_%d_%d_%d.mtx" % c["dims"]), *c["dims"])
        g = po.GMatrix.from_mtx(path)
        op = Operator(g)
    elif c["kind"] == "file":
        g = po.GMatrix.from_mtx(c["path"])
        op = Operator(g)
    else:
        g = po.GMatrix.generate(*c["dims"])
        scs = g.to_scs(64, 256)
        op = Operator(g, scs.oldToNewPerm.copy())
        scs.free()
    b = op.to_dev(g.rhs())
    eps = c["eps_rel"] * math.sqrt(po.ddot_tree(b, b))
    return op, b, c["m"], c["itermax"], eps


def run_case(name, tmpdir=None):
    op, b, m, itermax, eps = build_case(name, tmpdir)
    out = solve(op, b, m, itermax, eps)
    out["x"] = op.to_orig(out["x"])
    out["eps"] = eps
    out["bnorm"] = math.sqrt(po.ddot_tree(b, b))
    return out


def record(out):
    """what tests/golden/gmres_hist.json holds of a run: exact doubles as hex strings, x as a SHA-256 of its bytes"""
    return dict(k=int(out["k"]), res=[float(v).hex() for v in out["res"]], rr=[float(v).hex() for v in out["rr"]],
                x_sha256=hashlib.sha256(np.ascontiguousarray(out["x"], dtype=np.float64).tobytes()).hexdigest(),
                eps=float(out["eps"]).hex())


def unhex(a):
    return np.array([float.fromhex(v) for v in a])


def scipy_gap(name, ours, tmpdir=None):
    """max_k |res_ours[k] - res_scipy[k]| / ||b|| over the steps both solvers take (scipy.sparse.linalg.gmres, same restart
    length, callback_type="pr_norm": its estimate after every inner step, relative to ||b||)"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as sl
    op, b, m, itermax, eps = build_case(name, tmpdir)
    g = op.g
    A = sp.csr_matrix((g.val.copy(), g.col.astype(np.int64), g.rowPtr.astype(np.int64)), shape=(g.nr, g.nc))
    hist = []
    steps = max(itermax - 1, 1)
    sl.gmres(A, b, x0=np.zeros(len(b)), rtol=gmres_cases.CASES[name]["eps_rel"], atol=0.0, restart=m,
             maxiter=(steps + m - 1) // m, callback=hist.append, callback_type="pr_norm")
    mine = np.asarray(ours["res"][1:]) / ours["bnorm"]
    L = min(len(mine), len(hist))
    assert L >= len(mine) - 2 and L >= 1, (len(mine), len(hist))
    return float(np.max(np.abs(mine[:L] - np.asarray(hist[:L]))))
