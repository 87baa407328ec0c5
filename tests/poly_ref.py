"""The numerical contract of PCG with the Chebyshev polynomial preconditioner restated on the CPU: the bound on
lmax, the coefficients, the apply z = q(D^-1 A) D^-1 r, the two streaming kernels' lines, and `solve` -- pcg_ref.solve with
`z = r * dinv` replaced by the apply (sgs_ref.solve, which takes any plan with an `apply`).  TEST INFRASTRUCTURE ONLY.

Everything is in the DEVICE's row order (`op.to_dev`).  Every operation is rounded on its own: numpy elementwise operations, one
per rounding; the coefficients are Python floats computed in the contract's order.  tests/test_poly_host.py pins this
restatement before anything on the GPU is compared with it.
"""
import math

import numpy as np

from oracle import pyoracle as po

import pcg_ref
import sgs_ref
from sgs_ref import device_rows, probe_vector  # noqa: F401  (re-exported for the tests)
from pcg_ref import operator, same_bits, unhex, record, csr, gmatrix, problem_args  # noqa: F401

STEPS, RATIO, MAX_STEPS = 3, 16.0, 16


def coeffs(steps, lmax, ratio=RATIO):
    """dict(steps, lmin, lmax, c1, a, b): a[j], b[j] for j = 2 .. steps (entries 0, 1 unused), in the contract's order"""
    lmax, ratio = float(lmax), float(ratio)
    lmin = lmax / ratio
    theta = (lmax + lmin) * 0.5
    delta = (lmax - lmin) * 0.5
    sigma = theta / delta
    c1 = 1.0 / theta
    rho = 1.0 / sigma
    a, b = [0.0, 0.0], [0.0, 0.0]
    for _ in range(2, steps + 1):
        rj = 1.0 / (2.0 * sigma - rho)
        a.append(rj * rho)
        b.append((2.0 * rj) / delta)
        rho = rj
    return dict(steps=steps, lmin=lmin, lmax=lmax, c1=c1, a=a, b=b)


def coeff_array(c):
    """c1, then a_j, b_j pairs: what sb_pcg_poly_coeffs hands out"""
    out = [c["c1"]]
    for j in range(2, c["steps"] + 1):
        out += [c["a"][j], c["b"][j]]
    return np.array(out, dtype=np.float64)


def rowbound(g, op, dinv_dev):
    """g_i (device order): the sum, from +0.0 in storage order over the stored entries of row i, of (|a| * sd_i) * sd[col],
    sd = sqrt(dinv).  (Sell-C-sigma padding is a stored +0.0 whose term is +0.0: it changes no sum that starts from +0.0.)"""
    ptr, col, val = device_rows(g, op)
    n = len(ptr) - 1
    lens = np.diff(ptr)
    with np.errstate(all="ignore"):
        sd = np.sqrt(dinv_dev)
        s = np.zeros(n)
        for j in range(int(lens.max()) if n else 0):
            m = np.nonzero(lens > j)[0]
            e = ptr[m] + j
            s[m] = s[m] + (np.abs(val[e]) * sd[m]) * sd[col[e]]
    return s


def naive_bound(g):
    """the largest absolute row sum of D^-1 A: the bound NOT used (it is useless on a badly scaled symmetric matrix)"""
    rp = g.rowPtr.astype(np.int64)
    row = np.repeat(np.arange(g.nr), np.diff(rp))
    return float(np.max(np.bincount(row, weights=np.abs(g.val) * pcg_ref.jacobi(g)[row], minlength=g.nr)))


class Plan:
    """dinv (device order), the bound's row values, the coefficients; `apply` is the contract's"""

    def __init__(self, g, op, steps=STEPS, lmax=None, ratio=RATIO):
        self.op, self.n = op, g.nr
        self.dinv = op.to_dev(pcg_ref.jacobi(g))
        self.g = rowbound(g, op, self.dinv)
        self.c = coeffs(steps, float(np.max(self.g)) if lmax is None else lmax, ratio)
        self.steps = steps

    def apply(self, r, dinv=None):
        """(z, d) in device order of r in device order.  dinv: ignored unless given (sgs_ref.solve passes the handle's, the same)"""
        dinv = self.dinv if dinv is None else dinv
        c = self.c
        with np.errstate(all="ignore"):
            d = (r * dinv) * c["c1"]
            z = d.copy()
            for j in range(2, self.steps + 1):
                w = self.op.spmv(z)
                d, z = step(r, w, dinv, d, z, c["a"][j], c["b"][j])
        return z, d


def step(r, w, dinv, d, z, a, b):
    """step j >= 2 behind w = A z: the new (d, z)"""
    with np.errstate(all="ignore"):
        u = r - w
        u = u * dinv
        d = (np.float64(a) * d) + (np.float64(b) * u)
        return d, z + d


def step_l1(r, w, dinv, d, z, a, b):
    """poly_step_k: (d, z, the level-1 values of r.z)"""
    d, z = step(r, w, dinv, d, z, a, b)
    with np.errstate(all="ignore"):
        return d, z, po.ddot_partials(np.ascontiguousarray(r), z)


def update_r(r, Ap, dinv, nalpha, c1):
    """poly_update_r_k: r, d = z, the level-1 values of r.z and r.r"""
    with np.errstate(all="ignore"):
        rn = po.waxpby(1.0, r, float(nalpha), Ap)
        z = (rn * np.asarray(dinv, dtype=np.float64)) * np.float64(c1)
        return rn, z, po.ddot_partials(rn, z), po.ddot_partials(rn, rn)


def solve(op, plan, b_orig, itermax, eps, keep_x=False):
    """pcg_ref.solve with z = r * dinv replaced by the apply, in the prologue and in every body"""
    return sgs_ref.solve(op, plan, b_orig, op.to_orig(plan.dinv), itermax, eps, keep_x)


def build_case(c, tmpdir=None, steps=STEPS, lmax=None, ratio=RATIO):
    """(g, operator, plan, b, eps) of a case dict of poly_cases; b in original row order"""
    g = gmatrix(c["matrix"], tmpdir)
    op = operator(g, c["fmt"], c["C"], c["sigma"])
    b = g.rhs()
    eps = c["eps_rel"] * math.sqrt(po.ddot_tree(op.to_dev(b), op.to_dev(b)))
    return g, op, Plan(g, op, steps, lmax, ratio), b, eps


def run_case(c, tmpdir=None):
    g, op, plan, b, eps = build_case(c, tmpdir, c.get("steps", STEPS))
    out = solve(op, plan, b, c["itermax"], eps)
    out["eps"], out["dinv"], out["coeffs"] = eps, op.to_orig(plan.dinv), coeff_array(plan.c)
    g.free()
    return out


def dense_apply(plan):
    """the matrix of the apply, column by column (small n)"""
    n = plan.n
    M = np.zeros((n, n))
    for i in range(n):
        e = np.zeros(n)
        e[i] = 1.0
        M[:, i] = plan.apply(e)[0]
    return M
