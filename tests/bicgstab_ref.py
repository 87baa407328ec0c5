"""The numerical contract of right-preconditioned BiCGStab with a diagonal preconditioner restated on the CPU,
line for line, on top of the oracle's operations: `GMatrix.spmv` (through `gmres_ref.Operator`), `ddot_tree`, and numpy
elementwise operations (every product and every sum rounded on its own).  TEST INFRASTRUCTURE ONLY: lives in tests/, the product
never imports the oracle.

Vectors live in the DEVICE's row order (the permuted order of a Sell-C-sigma matrix with sigma > 1), which is the order the
tree dot walks.  tests/test_bicgstab_host.py pins this restatement -- true residuals with scipy's CSR product -- before
anything on the GPU is compared with it.
"""
import math
import os
import tempfile

import numpy as np

from oracle import pyoracle as po

import bicgstab_cases
from cg_batch_ref import operator  # gmres_ref.Operator in the device's row order of a format
from pcg_ref import csr, jacobi  # noqa: F401  (d by sb_matrix_diagonal's storage-order rule; 1.0 / d)

HISTORIES = ("rr", "rho", "rv", "ts", "tt")


def update_p(r, p, v, dinv, beta, omega):
    """p = r + beta * (p - omega * v), ph = p o dinv"""
    with np.errstate(all="ignore"):
        t1 = np.float64(omega) * v
        t2 = p - t1
        t3 = np.float64(beta) * t2
        pn = r + t3
        return pn, pn * dinv


def update_s(r, v, dinv, alpha):
    """s = r - alpha * v, sh = s o dinv"""
    with np.errstate(all="ignore"):
        t1 = np.float64(alpha) * v
        s = r - t1
        return s, s * dinv


def update_xr(x, ph, sh, s, t, alpha, omega):
    """x = (x + alpha * ph) + omega * sh, r = s - omega * t"""
    with np.errstate(all="ignore"):
        a1 = np.float64(alpha) * ph
        x1 = x + a1
        a2 = np.float64(omega) * sh
        xn = x1 + a2
        o1 = np.float64(omega) * t
        return xn, s - o1


def dot(a, b):
    return np.float64(po.ddot_tree(np.ascontiguousarray(a), np.ascontiguousarray(b)))


def solve(op, b_orig, dinv_orig, itermax, eps):
    """k, the five histories and x (original row order) of the BiCGStab contract with right-hand side b_orig and preconditioner
    dinv_orig (both in original row order)"""
    b = op.to_dev(np.asarray(b_orig, dtype=np.float64))
    dinv = op.to_dev(np.asarray(dinv_orig, dtype=np.float64))
    n = len(b)
    h = {name: [] for name in HISTORIES}
    with np.errstate(all="ignore"):
        x = np.zeros(n)
        r = b.copy()
        rhat = b.copy()
        p = np.zeros(n)
        v = np.zeros(n)
        beta = np.float64(0.0)
        omega = np.float64(0.0)
        rho = dot(rhat, r)
        rr = dot(r, r)
        normr = np.sqrt(rr)
        h["rr"].append(rr), h["rho"].append(rho)
        k = 1
        while k < itermax and normr > eps:
            p, ph = update_p(r, p, v, dinv, beta, omega)
            v = op.spmv(ph)
            rv = dot(rhat, v)
            alpha = rho / rv
            s, sh = update_s(r, v, dinv, alpha)
            t = op.spmv(sh)
            ts = dot(t, s)
            tt = dot(t, t)
            omega = ts / tt
            x, r = update_xr(x, ph, sh, s, t, alpha, omega)
            rho_old = rho
            rho = dot(rhat, r)
            rr = dot(r, r)
            normr = np.sqrt(rr)
            beta = (rho / rho_old) * (alpha / omega)
            h["rr"].append(rr), h["rho"].append(rho), h["rv"].append(rv), h["ts"].append(ts), h["tt"].append(tt)
            k += 1
    out = {name: np.array(a, dtype=np.float64) for name, a in h.items()}
    out["k"], out["x"] = k, op.to_orig(x)
    return out


def l1(a, b):
    """the level-1 values of a.b (one per aligned 256-element group) and their total"""
    q = po.ddot_partials(np.ascontiguousarray(a), np.ascontiguousarray(b))
    return q, po.reduce_final(q)


_dir = None


def matrix_path(matrix, tmpdir=None):
    global _dir
    if tmpdir is None:
        _dir = _dir or tempfile.mkdtemp(prefix="bicgstab_")
        tmpdir = _dir
    kind, dims = matrix[0], tuple(matrix[1:])
    path = os.path.join(str(tmpdir), "%s_%d_%d_%d.mtx" % ((kind,) + dims))
    if not os.path.exists(path):
        (bicgstab_cases.write_convdiff if kind == "cd" else bicgstab_cases.write_scaled_convdiff)(path, *dims)
    return path


def problem_args(matrix, tmpdir=None):
    """(filename, nx, ny, nz) for hostapi.Problem / the drivers"""
    kind = matrix[0]
    if kind == "hpcg":
        return "generate", matrix[1], matrix[1], matrix[1]
    if kind == "dims":
        return ("generate",) + tuple(matrix[1:])
    return matrix_path(matrix, tmpdir), 1, 1, 1


def gmatrix(matrix, tmpdir=None):
    if matrix[0] in ("hpcg", "dims"):
        return po.GMatrix.generate(*problem_args(matrix)[1:])
    return po.GMatrix.from_mtx(matrix_path(matrix, tmpdir))


def dinv_of(c, g):
    if c["precond"] == "jacobi":
        return jacobi(g)
    if c["precond"] == "none":
        return np.ones(g.nr)
    return bicgstab_cases.scale(np.arange(g.nr))


def build_case(c, tmpdir=None):
    """(g, operator, b, dinv, eps) of a case dict of bicgstab_cases; b and dinv in original row order"""
    g = gmatrix(c["matrix"], tmpdir)
    op = operator(g, c["fmt"], c["C"], c["sigma"])
    b = g.rhs()
    eps = c["eps_rel"] * math.sqrt(po.ddot_tree(op.to_dev(b), op.to_dev(b)))
    return g, op, b, dinv_of(c, g), eps


def run_case(c, tmpdir=None):
    g, op, b, dinv, eps = build_case(c, tmpdir)
    out = solve(op, b, dinv, c["itermax"], eps)
    out["eps"], out["dinv"], out["b"] = eps, dinv, b
    out["A"] = csr(g)
    g.free()
    return out
