"""solveCG (src/CGSolver.c:62-141) restated on the CPU for an ARBITRARY right-hand side, on top of the oracle's operations:
`GMatrix.spmv`, `waxpby`, `ddot_tree`.  This is what every column of a batched solve must reproduce bit for bit.
TEST INFRASTRUCTURE ONLY: lives in tests/, the product never imports the oracle.

Vectors live in the DEVICE's row order: for a Sell-C-sigma matrix with sigma > 1 that is the permuted order, which is the
order the tree dot walks (`gmres_ref.Operator`).  tests/test_cg_batch_host.py pins this restatement to `pyoracle.cg(dot="tree")`
and to tests/golden/cg_hist_tree.json before anything on the GPU is compared with it.
"""
import numpy as np

from oracle import pyoracle as po

from gmres_ref import Operator


def batch_rhs(b0, nrhs, start_row=0):
    """the right-hand sides of solveCGBatch: b_0 = b0; b_c[i] = b0[i] + c * ((g(i) mod 5) - 2), g the global row index
    (integers: exact)"""
    b0 = np.asarray(b0, dtype=np.float64)
    g = (np.arange(len(b0), dtype=np.int64) + int(start_row)) % 5 - 2
    return np.stack([b0 + float(c) * g.astype(np.float64) for c in range(nrhs)])


def operator(g, fmt="crs", Cc=64, sigma=1):
    """the operator in the device's row order of the given format"""
    if fmt == "scs" and sigma > 1:
        scs = g.to_scs(Cc, sigma)
        op = Operator(g, scs.oldToNewPerm.copy())
        scs.free()
        return op
    return Operator(g)


def solve(op, b_orig, itermax, eps):
    """k, rr, pAp, x (original row order) of solveCG with right-hand side b_orig (original row order), line for line"""
    b = op.to_dev(np.asarray(b_orig, dtype=np.float64))
    n = len(b)
    x = np.zeros(n)
    rr, pAp = [], []
    with np.errstate(all="ignore"):
        p = po.waxpby(1.0, x, 0.0, x)  # :94
        Ap = op.spmv(p)  # :96
        r = po.waxpby(1.0, b, -1.0, Ap)  # :97
        rtrans = np.float64(po.ddot_tree(r, r))  # :98
        rr.append(rtrans)
        normr = np.sqrt(rtrans)  # :100
        k = 1
        while k < itermax and normr > eps:  # :107
            if k == 1:
                p = po.waxpby(1.0, r, 0.0, r)  # :109
            else:
                oldrtrans = rtrans
                rtrans = np.float64(po.ddot_tree(r, r))  # :112
                rr.append(rtrans)
                beta = rtrans / oldrtrans  # :113
                p = po.waxpby(1.0, r, float(beta), p)  # :114
            normr = np.sqrt(rtrans)  # :116
            Ap = op.spmv(p)  # :123
            alpha = np.float64(po.ddot_tree(p, Ap))  # :125
            pAp.append(alpha)
            alpha = rtrans / alpha  # :126
            x = po.waxpby(1.0, x, float(alpha), p)  # :127
            r = po.waxpby(1.0, r, float(-alpha), Ap)  # :128
            k += 1
    return dict(k=k, rr=np.array(rr, dtype=np.float64), pAp=np.array(pAp, dtype=np.float64), x=op.to_orig(x))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
