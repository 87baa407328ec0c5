"""The numerical contract of right-preconditioned GMRES(m) restated on the CPU: GMRES on A M^-1 by a change of
variable.  The restatement IS `gmres_ref.solve`, unchanged, handed an operator whose `spmv(u)` is `op.spmv(plan.apply(u)[0])`; the
solution is xs = plan.apply(u)[0] of the u it returns.  A plan is `precond_ref.Hierarchy` built by
`bicgstab_precond_ref.build_plan` (the aggregation hierarchy: `aggregation_ref.build`), or a diagonal.  Nothing of either is copied.
Beside it: the two formulas of the kernels that write the first part of M^-1 of the vector they make, and the launch formula.
TEST INFRASTRUCTURE ONLY.

Vectors live in the DEVICE's row order.  tests/test_gmres_precond_host.py pins this restatement -- scipy's GMRES on the same
operator, true residuals with scipy's CSR product, the iteration counts of DESIGN 4.20's table -- before anything on the GPU is
compared with it.
"""
import hashlib
import math

import numpy as np

from oracle import pyoracle as po

import bicgstab_precond_ref as bpr
import bicgstab_ref as br
import gmres_precond_cases as cases
import gmres_ref
import precond_ref as pr


class Diagonal:
    """M^-1 = diag(dinv), device order; dinv None: the identity (no product at all)"""

    kind = 0

    def __init__(self, dinv_dev=None):
        self.dinv = None if dinv_dev is None else np.ascontiguousarray(dinv_dev, dtype=np.float64)

    def apply(self, r):
        with np.errstate(all="ignore"):
            return (np.array(r, dtype=np.float64) if self.dinv is None else first(r, self.dinv)), None

    def launches(self):
        return 0

    def free(self):
        pass


class RightPreconditioned:
    """u -> A (M^-1 u): what gmres_ref.solve takes for its operator"""

    def __init__(self, op, plan):
        self.op, self.plan = op, plan

    def spmv(self, u):
        return self.op.spmv(self.plan.apply(u)[0])


def first(v, dinv, c1=None):
    """what a producer of v also writes.  c1 None, a diagonal: v o dinv, all of M^-1 v.  Else the Chebyshev plans' step 1 on
    level 0: d = z = (v o dinv) * c1 (poly_first_k's arithmetic), every product rounded on its own"""
    with np.errstate(all="ignore"):
        t = np.asarray(v, dtype=np.float64) * np.asarray(dinv, dtype=np.float64)
        return t if c1 is None else t * np.float64(c1)


def is_cheb(plan):
    return plan.kind in (pr.POLY, pr.MGPOLY)


def apply_launches(plan):
    """A: launches of an apply beyond what rides in the fused loop: 0 for a diagonal, the cycle's less level 0's step 1 under the
    polynomial, the whole cycle's under the sweeps"""
    if plan.kind == 0:
        return 0
    return plan.launches() - (1 if is_cheb(plan) else 0)


def launches_per_step(plan, m, j):
    """sb_gmres_launches_per_step of a fused preconditioned handle: 7 + A, + 1 at j = 0, + 5 + A at j = m - 1"""
    A = apply_launches(plan)
    return 7 + A + (1 if j == 0 else 0) + (5 + A if j == m - 1 else 0)


def positions(m):
    """the cycle positions whose launches the golden file holds: the first, a middle one, the last"""
    return sorted({0, m // 2, m - 1})


def solve(op, plan, b_orig, m, itermax, eps):
    """k, res, rr, closes as gmres_ref.solve gives them on A M^-1; u (device order) and x = xs (ORIGINAL row order): M^-1 u of
    the last close, 0 when no step was taken"""
    b = op.to_dev(np.asarray(b_orig, dtype=np.float64))
    out = gmres_ref.solve(RightPreconditioned(op, plan), b, m, itermax, eps)
    u = out["x"]
    xs = plan.apply(u)[0] if len(out["rr"]) > 1 else np.zeros(len(b))
    out["u"], out["x"] = u, op.to_orig(xs)
    return out


def build_plan(c, tmpdir=None, coarse_csr=None):
    """(plan, operator of level 0, b in original order, eps) of a case dict of gmres_precond_cases"""
    p = c["precond"]
    if p in bpr.KINDS and not c.get("aggregation"):
        return bpr.build_plan(c, tmpdir, coarse_csr)
    g = br.gmatrix(c["matrix"], tmpdir)
    fmt = (c["fmt"], c["C"], c["sigma"])
    if c.get("aggregation"):
        import aggregation_cases as ac
        import aggregation_ref as ar
        return ar.build(g, fmt, steps=c["steps"], found=ac.levels_of(tuple(c["matrix"])))[:4]
    op = br.operator(g, *fmt)
    b = g.rhs()
    eps = c["eps_rel"] * math.sqrt(po.ddot_tree(op.to_dev(b), op.to_dev(b)))
    if p == "none":
        plan = Diagonal()
    elif p == "jacobi":
        plan = Diagonal(op.to_dev(br.jacobi(g)))
    elif p == "signed":
        plan = Diagonal(op.to_dev(cases.signed_scale(np.arange(g.nr))))
    else:
        raise ValueError("the cases have no %r" % (p,))
    plan.g = g
    return plan, op, b, eps


def level0(plan):
    return plan.lev[0].g if plan.kind else plan.g


def run_case(c, tmpdir=None, coarse_csr=None):
    plan, op, b, eps = build_plan(c, tmpdir, coarse_csr)
    out = solve(op, plan, b, c["m"], c["itermax"], eps)
    out["eps"], out["b"], out["A"] = eps, b, br.csr(level0(plan))
    out["bnorm"] = math.sqrt(po.ddot_tree(op.to_dev(b), op.to_dev(b)))
    out["launches"] = [launches_per_step(plan, c["m"], j) for j in positions(c["m"])]
    if plan.kind:
        plan.free()
    else:
        plan.g.free()
    return out


def record(out):
    """what tests/golden/gmres_precond_hist.json holds of a run: exact doubles as hex strings, x as a SHA-256 of its bytes"""
    rec = gmres_ref.record(out)
    rec["launches"] = [int(v) for v in out["launches"]]
    return rec


def x_sha256(x):
    return hashlib.sha256(np.ascontiguousarray(x, dtype=np.float64).tobytes()).hexdigest()


def true_residual_ratio(out):
    """||b - A xs|| / eps with scipy's CSR product, original row order"""
    r = out["b"] - out["A"] @ out["x"]
    return float(np.sqrt(r @ r)) / out["eps"]


def close_gap(out):
    """max over the cycle closes of |estimate - explicit residual norm| / ||b||"""
    return max(abs(est - true) for est, true in out["closes"]) / out["bnorm"]


def scipy_gap(c, ours, tmpdir=None):
    """max_k |res_ours[k] - res_scipy[k]| / ||b|| over the steps both take: scipy.sparse.linalg.gmres on the LinearOperator of
    A M^-1 (no M= argument), same restart, callback_type "pr_norm": its estimate after every inner step, relative to ||b||"""
    import scipy.sparse.linalg as sl
    plan, op, b, eps = build_plan(c, tmpdir)
    bd = op.to_dev(b)
    A = RightPreconditioned(op, plan)
    n = len(bd)
    lin = sl.LinearOperator((n, n), matvec=lambda u: A.spmv(np.ascontiguousarray(u, dtype=np.float64).ravel()), dtype=np.float64)
    hist = []
    steps = max(c["itermax"] - 1, 1)
    sl.gmres(lin, bd, x0=np.zeros(n), rtol=c["eps_rel"], atol=0.0, restart=c["m"], maxiter=(steps + c["m"] - 1) // c["m"],
             callback=hist.append, callback_type="pr_norm")
    if plan.kind:
        plan.free()
    else:
        plan.g.free()
    mine = np.asarray(ours["res"][1:]) / ours["bnorm"]
    L = min(len(mine), len(hist))
    assert L >= len(mine) - 2 and L >= 1, (len(mine), len(hist))
    return float(np.max(np.abs(mine[:L] - np.asarray(hist[:L]))))
