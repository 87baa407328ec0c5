"""The numerical contract of preconditioned CG on P ranks restated on the CPU, for the tests only: pcg_ref.solve
and precond_ref's polynomial, statement for statement, with every vector a list of the ranks' pieces.  Built from what exists:
the oracle's partition (oracle/pyoracle.py: GMatrix.generate / irregular_locs, Plans) and its operations (GMatrix.spmv, waxpby,
ddot_tree), pcg_ref's operator and diagonal, precond_ref's Chebyshev coefficients, step and row bound.  The product never
imports it.

  - a rank's vectors live in ITS device row order (`pcg_ref.operator` of its local matrix); an SpMV input carries the rank's
    halo entries behind its nr rows, delivered from the plans as src/comm.c:627-649 delivers them (sp_mpi_ref.halo_fill's rule);
  - every dot is the rank's own tree-order value over its nr rows in device order, then the pairwise tree over ranks in rank
    order, ((v0 + v1) + (v2 + v3)) + ..., an odd tail moving up unchanged (`rank_sum`);
  - the polynomial's row bound reads dinv at the halo columns, and lmax is the MAX over ranks.

tests/test_pcg_multirank_host.py pins this restatement before anything on the GPU is compared with it.
"""
import hashlib
import types

import numpy as np

from oracle import pyoracle as po

import pcg_ref
import precond_ref


def rank_sum(values):
    """pairwise tree in rank order; an odd tail moves up unchanged"""
    v = [np.float64(x) for x in values]
    with np.errstate(all="ignore"):
        while len(v) > 1:
            nxt = [v[i] + v[i + 1] for i in range(0, len(v) - 1, 2)]
            if len(v) & 1:
                nxt.append(v[-1])
            v = nxt
    return np.float64(v[0])


class Ranks:
    """P local matrices (oracle-owned; Plans rewrites their columns to local numbering, halo columns behind the nr rows), their
    halo plans and each rank's operator in the device row order of (fmt, Cc, sigma)"""

    def __init__(self, locs, fmt="crs", Cc=64, sigma=1):
        self.locs, self.P = locs, len(locs)
        self.plans = po.Plans(locs)
        self.plan = [self.plans.plan(r) for r in range(self.P)]
        self.ops = [pcg_ref.operator(g, fmt, Cc, sigma) for g in locs]
        self.fmt = (fmt, Cc, sigma)

    @classmethod
    def generate(cls, n, P, fmt="crs", Cc=64, sigma=1):
        return cls([po.GMatrix.generate(n, n, n, r, P) for r in range(P)], fmt, Cc, sigma)

    @classmethod
    def irregular(cls, n, P, fmt="crs", Cc=64, sigma=1):
        from irregular_locs import irregular_locs
        return cls(irregular_locs(n, P), fmt, Cc, sigma)

    def to_dev(self, vs):
        return [op.to_dev(np.asarray(v, dtype=np.float64)) for op, v in zip(self.ops, vs)]

    def to_orig(self, vs):
        return [op.to_orig(v) for op, v in zip(self.ops, vs)]

    def externals(self, vs_dev):
        """per rank the halo entries of the device-order vectors vs_dev: rank s's block for r is its elementsToSend (original
        local row numbers) in order, and lands at r's rdispl for s"""
        orig = self.to_orig(vs_dev)
        out = []
        for r, pl in enumerate(self.plan):
            ext = np.zeros(pl["externalCount"])
            for j in range(pl["indegree"]):
                s = int(pl["sources"][j])
                ps = self.plan[s]
                i = list(ps["destinations"]).index(r)
                idx = ps["elementsToSend"][ps["sdispls"][i]:ps["sdispls"][i] + ps["sendCounts"][i]]
                ext[pl["rdispls"][j]:pl["rdispls"][j] + pl["recvCounts"][j]] = orig[s][idx]
            out.append(ext)
        return out

    def spmv(self, vs_dev):
        """A v on every rank, device order: the halo exchange, then the local rows' sums in storage order"""
        ext = self.externals(vs_dev)
        return [op.to_dev(g.spmv(np.concatenate([op.to_orig(v), e]))) for g, op, v, e in zip(self.locs, self.ops, vs_dev, ext)]

    def dot(self, a, b):
        return rank_sum([po.ddot_tree(np.ascontiguousarray(x), np.ascontiguousarray(y)) for x, y in zip(a, b)])

    def rhs(self):
        """b per rank, original row order"""
        return [g.rhs() for g in self.locs]

    def norm_b(self):
        b = self.to_dev(self.rhs())
        return float(np.sqrt(self.dot(b, b)))

    def jacobi(self):
        """1 / diag of the rank's own rows, original row order (a local column i < nr is the rank's own row i)"""
        return [pcg_ref.jacobi(g) for g in self.locs]

    def rowbound(self, dinv_dev):
        """per rank g_i of its own rows, device order: precond_ref.rowbound over the local rows with dinv at the halo columns
        behind the rank's own (one halo exchange of dinv)"""
        ext = self.externals(dinv_dev)
        out = []
        for g, op, d, e in zip(self.locs, self.ops, dinv_dev, ext):
            nr, ne = g.nr, len(e)
            if op.o2n is None:
                wide = op
            else:  # device numbering of the columns: the rank's own rows permuted, the halo columns where they are
                wide = types.SimpleNamespace(o2n=np.concatenate([op.o2n, nr + np.arange(ne, dtype=np.int64)]), n2o=op.n2o)
            out.append(precond_ref.rowbound(g, wide, np.concatenate([d, e])))
        return out

    def lmax(self, dinv_dev):
        return float(max(float(np.max(v)) for v in self.rowbound(dinv_dev) if len(v)))

    def assemble_csr(self):
        """(rowPtr, col, val) of the global matrix, the ranks' rows in rank order, every row's entries in its storage order:
        local column c < nr is global row start + c, a halo column its plan's externalGlobal"""
        lens, cols, vals = [], [], []
        starts = np.concatenate(([0], np.cumsum([g.nr for g in self.locs])))
        for r, (g, pl) in enumerate(zip(self.locs, self.plan)):
            glob = np.concatenate([starts[r] + np.arange(g.nr, dtype=np.int64), pl["externalGlobal"].astype(np.int64)])
            lens.append(np.diff(g.rowPtr.astype(np.int64)))
            cols.append(glob[g.col.astype(np.int64)])
            vals.append(g.val.copy())
        return np.concatenate(([0], np.cumsum(np.concatenate(lens)))), np.concatenate(cols), np.concatenate(vals)

    def assemble(self):
        """the global matrix as scipy CSR"""
        import scipy.sparse as sp
        rp, col, val = self.assemble_csr()
        return sp.csr_matrix((val, col, rp), shape=(len(rp) - 1, len(rp) - 1))

    def free(self):
        for g in self.locs:
            g.free()


class Poly:
    """precond_ref.Cheb of kind 4 (no padding term) across the ranks: the coefficients of [lmax / ratio, lmax], lmax None: the
    MAX over ranks of the row bound; apply: step 1, then per step an SpMV with its halo exchange and precond_ref.step"""

    def __init__(self, R, dinv_dev, steps=None, lmax=None, ratio=None):
        self.R, self.dinv = R, dinv_dev
        self.steps = precond_ref.STEPS[precond_ref.POLY] if steps is None else steps
        self.g = R.rowbound(dinv_dev)
        self.c = precond_ref.coeffs(self.steps, R.lmax(dinv_dev) if lmax is None else lmax,
                                    precond_ref.RATIO[precond_ref.POLY] if ratio is None else ratio)

    def apply(self, r):
        with np.errstate(all="ignore"):
            d = [(x * di) * np.float64(self.c["c1"]) for x, di in zip(r, self.dinv)]
            z = [x.copy() for x in d]
            for j in range(2, self.steps + 1):
                w = self.R.spmv(z)
                nxt = [precond_ref.step(r[q], w[q], self.dinv[q], d[q], z[q], self.c["a"][j], self.c["b"][j]) for q in range(self.R.P)]
                d, z = [t[0] for t in nxt], [t[1] for t in nxt]
        return z


def solve(R, dinv_orig, itermax, eps, poly=None, keep_x=False):
    """pcg_ref.solve on R's ranks: k, rr, rz, pAp, x (per rank, original row order).  dinv_orig: per rank, original order.
    poly: None, or dict(steps, lmax, ratio) -- z is then the polynomial's apply with dinv (precond_ref.solve's place for it).
    keep_x: also `xs`, the ranks' iterates after every body joined in rank order"""
    P = R.P
    b = R.to_dev(R.rhs())
    dinv = R.to_dev(dinv_orig)
    plan = Poly(R, dinv, **poly) if poly is not None else None
    wax = lambda al, x, be, y: [po.waxpby(al, x[q], be, y[q]) for q in range(P)]  # noqa: E731
    make_z = (lambda r: plan.apply(r)) if plan else (lambda r: [r[q] * dinv[q] for q in range(P)])
    x = [np.zeros(len(v)) for v in b]
    rr, rz, pAp, xs = [], [], [], []
    with np.errstate(all="ignore"):
        p = wax(1.0, x, 0.0, x)
        Ap = R.spmv(p)
        r = wax(1.0, b, -1.0, Ap)
        z = make_z(r)
        rtrans = R.dot(r, r)
        rztrans = R.dot(r, z)
        rr.append(rtrans), rz.append(rztrans)
        normr = np.sqrt(rtrans)
        k = 1
        while k < itermax and normr > eps:
            if k == 1:
                p = wax(1.0, z, 0.0, z)
            else:
                oldrz = rztrans
                z = make_z(r)
                rztrans = R.dot(r, z)
                rtrans = R.dot(r, r)
                rr.append(rtrans), rz.append(rztrans)
                beta = rztrans / oldrz
                p = wax(1.0, z, float(beta), p)
            normr = np.sqrt(rtrans)
            Ap = R.spmv(p)
            alpha = R.dot(p, Ap)
            pAp.append(alpha)
            alpha = rztrans / alpha
            x = wax(1.0, x, float(alpha), p)
            if keep_x:
                xs.append(np.concatenate(R.to_orig(x)))
            r = wax(1.0, r, float(-alpha), Ap)
            k += 1
    f = lambda a: np.array(a, dtype=np.float64)  # noqa: E731
    out = dict(k=k, rr=f(rr), rz=f(rz), pAp=f(pAp), x=R.to_orig(x), xs=xs)
    if plan:
        out["interval"] = (plan.c["lmin"], plan.c["lmax"])
        out["coeffs"] = precond_ref.coeff_array(plan.c)
    return out


def update_r(R, r, Ap, dinv, nalpha):
    """the r update as the kernels take it on every rank (pcg_ref.update_r: r, z and the level-1 values of r.z and r.r, reduced
    by levels 1-2 to the rank's own sums), then the pairwise tree over ranks of each sum: (r, z, r.z, r.r)"""
    per = [pcg_ref.update_r(r[q], Ap[q], dinv[q], nalpha) for q in range(R.P)]
    return [t[0] for t in per], [t[1] for t in per], rank_sum([t[4] for t in per]), rank_sum([t[5] for t in per])


def caller_dinv(R):
    """the tests' caller's diagonal, non-constant and positive: Jacobi's times 1 + (g mod 4) / 8 of the GLOBAL row g (the factor
    is exact, the product rounded once); per rank, original row order"""
    starts = np.concatenate(([0], np.cumsum([g.nr for g in R.locs])))
    return [d * (1.0 + ((starts[r] + np.arange(len(d))) % 4) * 0.125) for r, d in enumerate(R.jacobi())]


# name -> what tests/golden/pcg_mpi_hist.json holds a run of: workload ("hpcg" | "irregular"), n, P, format, the preconditioner
# ("jacobi" | "caller" | "poly"), the solve
def _c(workload, n, P, fmt, C, sigma, precond, itermax, eps_rel, **poly):
    return dict(workload=workload, n=n, P=P, fmt=fmt, C=C, sigma=sigma, precond=precond, itermax=itermax, eps_rel=eps_rel, poly=poly or None)


CASES = {
    "hpcg16_x2_sell_64_256_jacobi": _c("hpcg", 16, 2, "scs", 64, 256, "jacobi", 60, 0.0),
    "hpcg16_x4_sell_64_1_caller": _c("hpcg", 16, 4, "scs", 64, 1, "caller", 60, 0.0),
    "hpcg16_x2_crs_poly3": _c("hpcg", 16, 2, "crs", 64, 1, "poly", 60, 0.0, steps=3),
    "hpcg8_x3_sell_4_8_poly3_lmax": _c("hpcg", 8, 3, "scs", 4, 8, "poly", 40, 0.0, steps=3, lmax=1.75),
    "irregular12_x3_crs_jacobi": _c("irregular", 12, 3, "crs", 64, 1, "jacobi", 100, 1e-10),
    "irregular12_x3_sell_64_256_poly1": _c("irregular", 12, 3, "scs", 64, 256, "poly", 100, 1e-10, steps=1),
}


def ranks_of(c):
    make = Ranks.irregular if c["workload"] == "irregular" else Ranks.generate
    return make(c["n"], c["P"], c["fmt"], c["C"], c["sigma"])


def dinv_of(c, R):
    return caller_dinv(R) if c["precond"] == "caller" else R.jacobi()


def run_case(c, keep_x=False):
    R = ranks_of(c)
    eps = c["eps_rel"] * R.norm_b()
    out = solve(R, dinv_of(c, R), c["itermax"], eps, poly=c["poly"], keep_x=keep_x)
    out["eps"] = eps
    R.free()
    return out


def record(out):
    """what the golden file holds of a run: exact doubles as hex strings, every rank's x as a SHA-256 of its bytes"""
    h = lambda a: [float(v).hex() for v in a]  # noqa: E731
    rec = dict(k=int(out["k"]), rr=h(out["rr"]), rz=h(out["rz"]), pAp=h(out["pAp"]), eps=float(out["eps"]).hex(),
               x_sha256=[hashlib.sha256(np.ascontiguousarray(x, dtype=np.float64).tobytes()).hexdigest() for x in out["x"]])
    if "interval" in out:
        rec["interval"] = h(out["interval"])
    return rec
