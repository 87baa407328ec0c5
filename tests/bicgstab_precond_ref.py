"""The numerical contract of right-preconditioned BiCGStab under a preconditioner plan restated on the CPU: the
loop of tests/bicgstab_ref.py -- its three update functions as they are -- with `ph = p o dinv` and `sh = s o dinv` replaced by
`Hierarchy.apply` of tests/precond_ref.py, the one restatement of PCG's preconditioners.  Nothing of either is copied.  TEST
INFRASTRUCTURE ONLY.

Vectors live in the DEVICE's row order.  tests/test_bicgstab_precond_host.py pins this restatement -- true residuals with scipy's
CSR product, the iteration counts of DESIGN 4.18's table -- before anything on the GPU is compared with it.
"""
import hashlib
import math

import numpy as np

from oracle import pyoracle as po

import bicgstab_ref as br
import precond_ref as pr

HISTORIES = br.HISTORIES
KINDS = {"sgs": pr.SGS, "mg": pr.MG, "mgfw": pr.MGFW, "poly": pr.POLY, "mgpoly": pr.MGPOLY}


def solve(op, plan, b_orig, itermax, eps):
    """k, the five histories and x (original row order): bicgstab_ref.solve with plan.apply in the two places"""
    b = op.to_dev(np.asarray(b_orig, dtype=np.float64))
    n = len(b)
    one = np.ones(n)  # the update functions' product with dinv is not used
    h = {name: [] for name in HISTORIES}
    with np.errstate(all="ignore"):
        x = np.zeros(n)
        r = b.copy()
        rhat = b.copy()
        p = np.zeros(n)
        v = np.zeros(n)
        beta = np.float64(0.0)
        omega = np.float64(0.0)
        rho = br.dot(rhat, r)
        rr = br.dot(r, r)
        normr = np.sqrt(rr)
        h["rr"].append(rr), h["rho"].append(rho)
        k = 1
        while k < itermax and normr > eps:
            p = br.update_p(r, p, v, one, beta, omega)[0]
            ph = plan.apply(p)[0]
            v = op.spmv(ph)
            rv = br.dot(rhat, v)
            alpha = rho / rv
            s = br.update_s(r, v, one, alpha)[0]
            sh = plan.apply(s)[0]
            t = op.spmv(sh)
            ts = br.dot(t, s)
            tt = br.dot(t, t)
            omega = ts / tt
            x, r = br.update_xr(x, ph, sh, s, t, alpha, omega)
            rho_old = rho
            rho = br.dot(rhat, r)
            rr = br.dot(r, r)
            normr = np.sqrt(rr)
            beta = (rho / rho_old) * (alpha / omega)
            h["rr"].append(rr), h["rho"].append(rho), h["rv"].append(rv), h["ts"].append(ts), h["tt"].append(tt)
            k += 1
    out = {name: np.array(a, dtype=np.float64) for name, a in h.items()}
    out["k"], out["x"] = k, op.to_orig(x)
    return out


def plan_update(xn, dinv, c1):
    """what the two plan kernels add with CHEB = 1 to the p (s) they have just made: d = (p o dinv) * c1, which is ph (sh) too"""
    with np.errstate(all="ignore"):
        return (xn * dinv) * np.float64(c1)


def dims_of(matrix):
    return (matrix[1],) * 3 if matrix[0] == "hpcg" else tuple(matrix[1:])


def build_plan(c, tmpdir=None, coarse_csr=None):
    """(Hierarchy, operator of level 0, b in original order, eps) of a case dict of bicgstab_precond_cases.  mgpoly: the trilinear
    P on every level; the coarse matrices are `coarse_csr` ((ptr, col, val) per level: a product formed elsewhere), or with
    `galerkin` scipy's P^T A P at omega = 1, or the stencil regenerated at omega = 0.25"""
    g = br.gmatrix(c["matrix"], tmpdir)
    fmt = (c["fmt"], c["C"], c["sigma"])
    kind = KINDS[c["precond"]]
    levels, transfers = [(g, br.operator(g, *fmt))], []
    if kind == pr.MGPOLY:
        dims = dims_of(c["matrix"])
        galerkin = c.get("galerkin") or coarse_csr is not None
        A = br.csr(g) if galerkin and coarse_csr is None else None
        for l in range(pr.geometric_levels(dims, c.get("levels")) - 1):
            P = pr.trilinear(dims)
            transfers.append((P, 1.0 if galerkin else pr.OMEGA[kind]))
            dims = tuple(d // 2 for d in dims)
            if coarse_csr is not None:
                ptr, col, val = coarse_csr[l]
                gc = po.GMatrix.from_csr(np.asarray(ptr).astype(np.uint32), np.asarray(col).astype(np.uint32),
                                         np.asarray(val, dtype=np.float64), nc=len(ptr) - 1)
            elif galerkin:
                import scipy.sparse as sp
                gc, A = pr.galerkin_gmatrix(A, sp.csr_matrix((P[2], P[1], P[0]), shape=(A.shape[0], dims[0] * dims[1] * dims[2])))
            else:
                gc = br.gmatrix(("dims",) + dims, tmpdir)
            levels.append((gc, br.operator(gc, *fmt)))
    elif kind not in (pr.SGS, pr.POLY):
        raise ValueError("the cases have no %r" % (c["precond"],))
    hier = pr.Hierarchy(kind, levels, transfers, c.get("steps"), c.get("coarse_steps"), c.get("lmax"), c.get("ratio"), fmt)
    op = hier.lev[0].op
    b = g.rhs()
    eps = c["eps_rel"] * math.sqrt(po.ddot_tree(op.to_dev(b), op.to_dev(b)))
    return hier, op, b, eps


def run_case(c, tmpdir=None, coarse_csr=None):
    hier, op, b, eps = build_plan(c, tmpdir, coarse_csr)
    out = solve(op, hier, b, c["itermax"], eps)
    out["eps"], out["b"], out["A"] = eps, b, br.csr(hier.lev[0].g)
    out["launches"] = launches_per_body(hier)
    hier.free()
    return out


def launches_per_body(hier):
    """10 + 2 C under the sweeps, 8 + 2 C under the polynomial (level 0's step 1 counts among C and rides in the two updates)"""
    return (8 if hier.kind in (pr.POLY, pr.MGPOLY) else 10) + 2 * hier.launches()


def record(out):
    """what tests/golden/bicgstab_precond_hist.json holds of a run: exact doubles as hex strings, x as a SHA-256 of its bytes"""
    h = lambda a: [float(v).hex() for v in a]  # noqa: E731
    rec = {name: h(out[name]) for name in HISTORIES}
    rec.update(k=int(out["k"]), eps=float(out["eps"]).hex(), launches=int(out["launches"]),
               x_sha256=hashlib.sha256(np.ascontiguousarray(out["x"], dtype=np.float64).tobytes()).hexdigest())
    return rec
