"""The numerical contract of preconditioned CG restated on the CPU, line for line, on top of the oracle's
operations: `GMatrix.spmv` (through `gmres_ref.Operator`), `waxpby`, `ddot_tree`; z = r * dinv is a numpy elementwise product
(one rounded multiply).  TEST INFRASTRUCTURE ONLY: lives in tests/, the product never imports the oracle.

Vectors live in the DEVICE's row order (the permuted order of a Sell-C-sigma matrix with sigma > 1), which is the order the
tree dot walks.  tests/test_pcg_host.py pins this restatement -- to the restatement of solveCG with dinv = 1, to scipy's
preconditioned CG, to tests/golden/pcg_hist.json -- before anything on the GPU is compared with it.
"""
import hashlib
import math
import os
import tempfile

import numpy as np

from oracle import pyoracle as po

import pcg_cases
from cg_batch_ref import operator, same_bits  # noqa: F401  (re-exported for the tests)


def diagonal(g):
    """d in ORIGINAL row order: the sum, in storage order from +0.0, of row i's stored entries whose column is i.  (A
    Sell-C-sigma copy stores the same entries in the same order and pads with +0.0, which changes no sum that starts from
    +0.0.)  No test matrix stores a diagonal entry twice."""
    rp, col, val = g.rowPtr.astype(np.int64), g.col.astype(np.int64), g.val
    d = np.zeros(g.nr)
    with np.errstate(all="ignore"):
        for i in range(g.nr):
            s = np.float64(0.0)
            for k in range(rp[i], rp[i + 1]):
                if col[k] == i:
                    s = s + val[k]
            d[i] = s
    return d


def jacobi(g):
    """dinv_i = 1.0 / d_i: one IEEE division; original row order"""
    with np.errstate(all="ignore"):
        return 1.0 / diagonal(g)


def solve(op, b_orig, dinv_orig, itermax, eps, keep_x=False):
    """k, rr, rz, pAp, x (original row order) of the PCG contract with right-hand side b_orig and preconditioner dinv_orig
    (both in original row order); keep_x: also `xs`, the iterate after every body"""
    b = op.to_dev(np.asarray(b_orig, dtype=np.float64))
    dinv = op.to_dev(np.asarray(dinv_orig, dtype=np.float64))
    n = len(b)
    x = np.zeros(n)
    rr, rz, pAp, xs = [], [], [], []
    with np.errstate(all="ignore"):
        p = po.waxpby(1.0, x, 0.0, x)
        Ap = op.spmv(p)
        r = po.waxpby(1.0, b, -1.0, Ap)
        z = r * dinv
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
                z = r * dinv
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


def update_r(r, Ap, dinv, nalpha):
    """the three lines the fused kernel takes: r, z, the level-1 values of r.z and r.r, and their totals"""
    with np.errstate(all="ignore"):
        rn = po.waxpby(1.0, r, float(nalpha), Ap)
        z = rn * np.asarray(dinv, dtype=np.float64)
        l1rz, l1rr = po.ddot_partials(rn, z), po.ddot_partials(rn, rn)
        return rn, z, l1rz, l1rr, po.reduce_final(l1rz), po.reduce_final(l1rr)


_scaled_dir = None


def scaled_path(n, tmpdir=None):
    global _scaled_dir
    if tmpdir is None:
        _scaled_dir = _scaled_dir or tempfile.mkdtemp(prefix="pcg_scaled_")
        tmpdir = _scaled_dir
    path = os.path.join(str(tmpdir), "scaled_hpcg_%d.mtx" % n)
    if not os.path.exists(path):
        pcg_cases.write_scaled_hpcg(path, n)
    return path


def irregular_matrix(n):
    """the irregular stand-in as the host library generates it, handed to the oracle"""
    from sparsebench_amd import hostapi
    p = hostapi.Problem("irregular", n, n, n, fmt="crs", upload=False)
    col, val = p.gm_entries()
    g = po.GMatrix.from_csr(p.array("rowPtr").copy(), col, val, nc=p.nc)
    p.free()
    return g


def problem_args(matrix, tmpdir=None):
    """(filename, nx, ny, nz) for hostapi.Problem / the drivers"""
    kind = matrix[0]
    if kind == "hpcg":
        return "generate", matrix[1], matrix[1], matrix[1]
    if kind == "dims":
        return ("generate",) + tuple(matrix[1:])
    if kind == "scaled":
        return scaled_path(matrix[1], tmpdir), 1, 1, 1
    if kind == "irregular":
        return "irregular", matrix[1], matrix[1], matrix[1]
    return matrix[1], 1, 1, 1


def gmatrix(matrix, tmpdir=None):
    kind = matrix[0]
    if kind in ("hpcg", "dims"):
        return po.GMatrix.generate(*problem_args(matrix)[1:])
    if kind == "irregular":
        return irregular_matrix(matrix[1])
    return po.GMatrix.from_mtx(problem_args(matrix, tmpdir)[0])


def dinv_of(c, g):
    if c["dinv"] == "jacobi":
        return jacobi(g)
    if c["dinv"] == "identity":
        return np.ones(g.nr)
    return pcg_cases.scale(np.arange(g.nr))


def build_case(c, tmpdir=None):
    """(g, operator, b, dinv, eps) of a case dict of pcg_cases; b and dinv in original row order"""
    g = gmatrix(c["matrix"], tmpdir)
    op = operator(g, c["fmt"], c["C"], c["sigma"])
    b = g.rhs()
    eps = c["eps_rel"] * math.sqrt(po.ddot_tree(op.to_dev(b), op.to_dev(b)))
    return g, op, b, dinv_of(c, g), eps


def run_case(c, tmpdir=None):
    g, op, b, dinv, eps = build_case(c, tmpdir)
    out = solve(op, b, dinv, c["itermax"], eps)
    out["eps"], out["dinv"] = eps, dinv
    g.free()
    return out


def record(out):
    """what tests/golden/pcg_hist.json holds of a run: exact doubles as hex strings, x as a SHA-256 of its bytes"""
    h = lambda a: [float(v).hex() for v in a]  # noqa: E731
    return dict(k=int(out["k"]), rr=h(out["rr"]), rz=h(out["rz"]), pAp=h(out["pAp"]),
                x_sha256=hashlib.sha256(np.ascontiguousarray(out["x"], dtype=np.float64).tobytes()).hexdigest(), eps=float(out["eps"]).hex())


def unhex(a):
    return np.array([float.fromhex(v) for v in a])


def csr(g):
    import scipy.sparse as sp
    return sp.csr_matrix((g.val.copy(), g.col.astype(np.int64), g.rowPtr.astype(np.int64)), shape=(g.nr, g.nc))
