"""The numerical contract of PCG's preconditioners restated once on the CPU, in the device plan's vocabulary:
a kind (sgs = 1, mg = 2, mgfw = 3, poly = 4, mgpoly = 5), per level a smoother (`Sweeps` or `Cheb`) and between neighbours a
transfer (`Injection` or `FullWeighting`), one `Hierarchy.cycle` that makes z for every kind, and `solve` -- pcg_ref.solve with
`z = r * dinv` replaced by the cycle.  SGS and the polynomial are the one-level cases.  TEST INFRASTRUCTURE ONLY.

Everything is in each level's DEVICE row order (`op.to_dev`).  Every operation is rounded on its own; double precision, tree dot
order; the Chebyshev coefficients are Python floats computed in the contract's order.

  V(l, r):
    1  z = the smoother from zero
         Sweeps: forward over colours 0 .. nC-1, row i: s = r_i ; lower(i) in storage order: s = s - a_e z[col_e] ; t_i = s ;
                 z_i = s * dinv_i ;  backward over nC-2 .. 0, row i: s = t_i ; upper(i): s = s - a_e z[col_e] ; z_i = s * dinv_i
         Cheb:   d = (r * dinv) * c1 ; z = d ;  for j = 2 .. steps: w = A_l z ; u = r - w ; u = u * dinv ; d = a_j d + b_j u ; z = z + d
    2  if l = L-1: return z
    3  rc = the transfer's restriction of the residual of (r, z)
         Injection, coarse row c injected from f:  s = r_f ; every stored entry e of row f with val_e != 0.0 in storage order, the
                 diagonal included: s = s - a_e z[col_e] ;  rc_c = s
         FullWeighting, coarse row c:  s = +0.0 ; the entries of row c of P_l^T with w_e != 0.0 in ascending ORIGINAL fine row:
                 s = s + w_e * d[row_e] ;  rc_c = omega_l * s, where the smoother says what d is --
                 Sweeps: a vector, row i: s = r_i ; lower(i): s = s - a_e z[col_e] ; upper(i) likewise ; d_i = s - diag_i * z_i
                 Cheb:   no vector, per entry u = r[row_e] - w[row_e] with w = A_l z
    4  zc = V(l+1, rc)
    5  Injection: z_f = z_f + zc_c.  FullWeighting, every fine row i with a kept entry in P_l: s = +0.0 ; its entries with
       w_e != 0.0 in storage order: s = s + w_e * zc[col_e] ; z_i = z_i + s  (other rows untouched)
    6  z = the smoother from the guess z
         Sweeps: forward, row i: s = r_i ; lower(i) ; t_i = s ; upper(i) ; z_i = s * dinv_i ;  backward as in 1
         Cheb:   w = A_l z ; u = r - w ; u = u * dinv ; d = u * c1 ; z = z + d ;  then steps 2 .. as in 1

tests/test_{sgs,mg,mg_fw,poly,mg_poly}_host.py pin this restatement before anything on the GPU is compared with it.
"""
import math

import numpy as np

from oracle import pyoracle as po

import pcg_ref
from pcg_ref import csr, gmatrix, operator

SGS, MG, MGFW, POLY, MGPOLY = 1, 2, 3, 4, 5  # the device plan's kinds
AUTO_DEPTH = 4  # HPCG's
STEPS = {POLY: 3, MGPOLY: 2}
RATIO = {POLY: 16.0, MGPOLY: 4.0}
# with the trilinear P and the stencil regenerated on the coarser grid: P^T A_h P ~ 2 A_H asks for 0.5, which mgfw keeps; mgpoly
# takes DESIGN 4.16's experiment's 0.25, and 1.0 on the Galerkin hierarchy
OMEGA = {MGFW: 0.5, MGPOLY: 0.25}


# ---- rows, rectangles and the one fold

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


def rect(row, col, val, n):
    """(len, col[n, w], val[n, w]) of entries already grouped by ascending `row`, their order within a row kept"""
    ln = np.bincount(row, minlength=n)
    start = np.concatenate(([0], np.cumsum(ln)))
    pos = np.arange(len(row)) - start[row]
    w = int(ln.max()) if len(ln) else 0
    cc, vv = np.zeros((n, w), dtype=np.int64), np.zeros((n, w))
    cc[row, pos], vv[row, pos] = col, val
    return ln, cc, vv


def take(R, rows):
    """the rectangle of the chosen rows alone, as narrow as they allow"""
    ln, cc, vv = R
    ln = ln[rows]
    w = int(ln.max()) if len(rows) else 0
    return ln, cc[rows][:, :w], vv[rows][:, :w]


def fold(s, v, R, sub=False):
    """s = s + a * v[col] (sub: s = s - a * v[col]) down the rectangle R, entry by entry in storage order, rows side by side;
    s is changed in place"""
    ln, cc, vv = R
    for j in range(cc.shape[1]):
        m = ln > j
        s[m] = s[m] - vv[m, j] * v[cc[m, j]] if sub else s[m] + vv[m, j] * v[cc[m, j]]
    return s


def chunk_longest(lens, C):
    """per chunk of C rows, the longest row: what Sell-C pads every row of the chunk to"""
    nch = (len(lens) + C - 1) // C
    padded = np.zeros(nch * C, dtype=np.int64)
    padded[:len(lens)] = lens
    return padded.reshape(nch, C).max(axis=1)


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
    kc, tr, kp, tp = kcol.tolist(), row[order].tolist(), kptr.tolist(), tptr.tolist()
    colour = [0] * n
    for i in range(n):
        taken = {colour[j] for j in kc[kp[i]:kp[i + 1]] if j < i}
        taken.update(colour[j] for j in tr[tp[i]:tp[i + 1]] if j < i)
        c = 0
        while c in taken:
            c += 1
        colour[i] = c
    return np.array(colour, dtype=np.int64)


# ---- the smoothers: pre(r) -> (z, aux) from zero, post(r, z) -> (z, aux) from the guess, residual(r, z) for full weighting

class Sweeps:
    """the multicoloured symmetric Gauss-Seidel sweep of a level: colour, nC, per colour the rows (ascending), and the lower and
    upper halves of the kept entries as rectangles (whole, and cut per colour); aux is t"""

    def __init__(self, V):
        ptr, col, val = device_rows(V.g, V.op)
        self.n, self.dinv, self.diag = V.n, V.dinv, V.diag
        self.kptr, self.kcol, self.kval = kept(ptr, col, val)
        self.colour = colouring(self.kptr, self.kcol)
        self.nC = int(self.colour.max()) + 1 if self.n else 0
        row = np.repeat(np.arange(self.n), np.diff(self.kptr))
        ci, cj = self.colour[row], self.colour[self.kcol]
        assert not np.any(ci == cj), "adjacent rows share a colour"
        self.rows = [np.nonzero(self.colour == c)[0] for c in range(self.nC)]
        self.half = [rect(row[sel], self.kcol[sel], self.kval[sel], self.n) for sel in (cj < ci, cj > ci)]
        self.cut = [[take(h, rows) for rows in self.rows] for h in self.half]

    def lower(self, i):
        return self._entries(i, 0)

    def upper(self, i):
        return self._entries(i, 1)

    def _entries(self, i, h):
        ln, cc, vv = self.half[h]
        return cc[i, :ln[i]], vv[i, :ln[i]]

    def pre(self, r):
        z, t = np.zeros(self.n), np.zeros(self.n)
        for c, rows in enumerate(self.rows):
            s = fold(r[rows], z, self.cut[0][c], sub=True)
            t[rows] = s
            z[rows] = s * self.dinv[rows]
        return self._backward(z, t)

    def post(self, r, z):
        """z is changed in place"""
        t = np.zeros(self.n)
        for c, rows in enumerate(self.rows):
            s = fold(r[rows], z, self.cut[0][c], sub=True)
            t[rows] = s
            z[rows] = fold(s, z, self.cut[1][c], sub=True) * self.dinv[rows]
        return self._backward(z, t)

    def _backward(self, z, t):
        for c in range(self.nC - 2, -1, -1):
            rows = self.rows[c]
            z[rows] = fold(t[rows], z, self.cut[1][c], sub=True) * self.dinv[rows]
        return z, t

    def residual(self, r, z):
        """d: the lower half, then the upper half, the diagonal last (no row reads another's d: all colours at once)"""
        s = fold(fold(r.copy(), z, self.half[0], sub=True), z, self.half[1], sub=True)
        return s - self.diag * z

    def launches(self):
        """of pre and of post alike: a kernel per colour and direction, the last colour's backward one folded away"""
        return 2 * self.nC - 1, 2 * self.nC - 1


def apply_scalar(sw, r, dinv):
    """Sweeps.pre entry by entry, as the contract words it (small matrices: pins the vectorised one above)"""
    n = sw.n
    z, t = np.zeros(n), np.zeros(n)
    with np.errstate(all="ignore"):
        for c in range(sw.nC):
            for i in sw.rows[c]:
                s = np.float64(r[i])
                for col, a in zip(*sw.lower(i)):
                    s = s - a * z[col]
                t[i] = s
                z[i] = s * dinv[i]
        for c in range(sw.nC - 2, -1, -1):
            for i in sw.rows[c]:
                s = np.float64(t[i])
                for col, a in zip(*sw.upper(i)):
                    s = s - a * z[col]
                z[i] = s * dinv[i]
    return z


def coeffs(steps, lmax, ratio=RATIO[POLY]):
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


def step(r, w, dinv, d, z, a, b):
    """Chebyshev step j >= 2 behind w = A z: the new (d, z)"""
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


class Cheb:
    """the Chebyshev smoother of a level: the bound's row values g, the coefficients c, `steps` of them; aux is d.

    pad: whether A z carries the Sell-C-sigma padding's term.  The format pads every row to its chunk's longest with (column 0,
    value 0.0) and the kernels multiply the padding, so a padded row's sum ends with + 0.0 * z[0] (device row 0).
    That changes nothing while z[0] is finite and the sum is not -0.0; a NaN or an inf in z[0] reaches every padded row.  The
    cycle (kind 5) is restated with the term, because the probes' NaN does get there; the polynomial handle (kind 4) is restated
    without it, on the oracle's row sums.  The two are kept apart on purpose."""

    def __init__(self, V, steps, lmax, ratio, pad):
        self.op, self.dinv, self.steps = V.op, V.dinv, steps
        self.g = rowbound(V.g, V.op, V.dinv)
        self.c = coeffs(steps, float(np.max(self.g)) if lmax is None else lmax, ratio)
        self.pad = None  # the device rows shorter than their chunk's longest
        if pad and V.fmt[0] == "scs":
            lens, C = np.diff(device_rows(V.g, V.op)[0]), V.fmt[1]
            self.pad = lens < np.repeat(chunk_longest(lens, C), C)[:V.n]

    def spmv(self, x):
        w = self.op.spmv(x)
        if self.pad is not None and self.pad.any():
            w[self.pad] = w[self.pad] + np.float64(0.0) * x[0]  # once: adding it again changes nothing
        return w

    def pre(self, r):
        d = (r * self.dinv) * np.float64(self.c["c1"])
        return self._steps(r, d, d.copy())

    def first(self, r, w, z):
        """step 1 from a guess behind w = A z: (d, z)"""
        u = r - w
        u = u * self.dinv
        d = u * np.float64(self.c["c1"])
        return d, z + d

    def post(self, r, z):
        d, z = self.first(r, self.spmv(z), z)
        return self._steps(r, d, z)

    def _steps(self, r, d, z):
        for j in range(2, self.steps + 1):
            d, z = step(r, self.spmv(z), self.dinv, d, z, self.c["a"][j], self.c["b"][j])
        return z, d

    def residual(self, r, z):
        """r - w with w = A z.  The device forms u = r[row_e] - w[row_e] per entry of P^T and keeps no vector; one rounding of
        the same two operands either way, so the gathered difference is the per-entry one bit for bit"""
        return r - self.spmv(z)

    def launches(self):
        """of pre (level 0's step 1, which rides in the r update, among them) and of post: an SpMV and a step kernel per step"""
        return 2 * self.steps - 1, 2 * self.steps


# ---- the transfers: restrict(V, r, z) -> rc and prolong(z, zc), z changed in place

class Injection:
    """f2c: coarse original row -> fine original row, translated through both permutations into `fine`; the stored non-zero
    entries of those fine rows, the diagonal included, as a rectangle"""
    launches = 2

    def __init__(self, V, f2c, coarse):
        f2c = np.asarray(f2c, dtype=np.int64)
        assert coarse.n == len(f2c) < V.n and len(np.unique(f2c)) == len(f2c) and f2c.min() >= 0 and f2c.max() < V.n
        self.fine = np.empty(len(f2c), dtype=np.int64)  # per coarse device row: the fine device row it is injected from
        self.fine[np.arange(len(f2c)) if coarse.op.o2n is None else coarse.op.o2n] = f2c if V.op.o2n is None else V.op.o2n[f2c]
        ptr, col, val = device_rows(V.g, V.op)
        row, keep = np.repeat(np.arange(V.n), np.diff(ptr)), val != 0.0
        self.stored = take(rect(row[keep], col[keep], val[keep], V.n), self.fine)

    def restrict(self, V, r, z):
        return fold(r[self.fine], z, self.stored, sub=True)

    def prolong(self, z, zc):
        z[self.fine] = z[self.fine] + zc
        return z


class FullWeighting:
    """P: (ptr, col, val), n_l x n_{l+1}, original numbering on both sides, translated through both permutations; the restriction
    is omega P^T of what the level's smoother calls the residual"""
    launches = 3  # the residual (Sweeps) or w = A z (Cheb), the restriction, the prolongation

    def __init__(self, V, P, omega, coarse):
        ptr, col, val = (np.asarray(a) for a in P)
        ptr, col, val = ptr.astype(np.int64), col.astype(np.int64), val.astype(np.float64)
        nc = coarse.n
        assert nc < V.n == len(ptr) - 1 and np.all(np.diff(ptr) >= 0) and (len(col) == 0 or (col.min() >= 0 and col.max() < nc))
        assert np.isfinite(val).all() and np.isfinite(omega) and omega > 0.0
        row = np.repeat(np.arange(V.n), np.diff(ptr))  # ascending original fine row, storage order within
        keep = val != 0.0
        row, col, val = row[keep], col[keep], val[keep]
        fdev = row if V.op.o2n is None else V.op.o2n[row]
        cdev = col if coarse.op.o2n is None else coarse.op.o2n[col]
        o = np.argsort(fdev, kind="stable")  # P: a row's entries in storage order
        self.P = rect(fdev[o], cdev[o], val[o], V.n)
        o = np.argsort(cdev, kind="stable")  # P^T: a coarse row's entries in ascending original fine row
        self.PT = rect(cdev[o], fdev[o], val[o], nc)
        self.omega, self.nc = float(omega), nc

    def weigh(self, d):
        return self.omega * fold(np.zeros(self.nc), d, self.PT)

    def restrict(self, V, r, z):
        return self.weigh(V.smoother.residual(r, z))

    def prolong(self, z, zc):
        """only the rows with a kept entry"""
        s, m = fold(np.zeros(len(z)), zc, self.P), self.P[0] > 0
        z[m] = z[m] + s[m]
        return z

    def bytes(self):
        """both Sell-64 structures as one cycle reads them: 12 B per padded element, 64 row lengths and 12 B per chunk"""
        longest = [chunk_longest(R[0], 64) for R in (self.PT, self.P)]
        return sum(12.0 * int(m.sum()) * 64 + len(m) * (64.0 * 4 + 12.0) for m in longest)


# ---- the levels and the one cycle

class Level:
    def __init__(self, g, op, fmt):
        self.g, self.op, self.n, self.fmt = g, op, g.nr, fmt
        self.diag, self.dinv = op.to_dev(pcg_ref.diagonal(g)), op.to_dev(pcg_ref.jacobi(g))
        self.smoother = self.transfer = None  # the transfer to the next level: none on the last

    def spmv_bytes(self):
        """sb_matrix_spmv_bytes of this level's matrix in the operator's format"""
        g = self.g
        if self.fmt[0] == "crs":
            return 12.0 * int(g.rowPtr[g.nr]) + 4.0 * (g.nr + 1) + 8.0 * g.nr + 8.0 * g.nc
        C = self.fmt[1]
        longest = chunk_longest(np.diff(device_rows(g, self.op)[0]), C)
        return 12.0 * int(longest.sum()) * C + 8.0 * len(longest) + 8.0 * len(longest) * C + 8.0 * g.nc


class Hierarchy:
    """kind: 1 .. 5; levels: [(g, op), ...] from fine to coarse (one level for sgs and poly); transfers: per level but the last
    an injection map f2c (mg) or (P, omega) (mgfw, mgpoly), original numbering on both sides; steps, coarse_steps (the last
    level's), lmax, ratio: the Chebyshev kinds'; fmt: (format, C, sigma) the operators were made with, for the padding's term and
    the byte model"""

    def __init__(self, kind, levels, transfers=(), steps=None, coarse_steps=None, lmax=None, ratio=None, fmt=("crs", 64, 1)):
        assert len(transfers) == len(levels) - 1 and (kind not in (SGS, POLY) or len(levels) == 1)
        self.kind, self.L = kind, len(levels)
        self.lev = [Level(g, op, fmt) for g, op in levels]
        if kind in (POLY, MGPOLY):
            self.steps = STEPS[kind] if steps is None else steps
            self.coarse_steps = self.steps if coarse_steps is None else coarse_steps
            ratio = RATIO[kind] if ratio is None else ratio
        for l, V in enumerate(self.lev):
            if kind in (POLY, MGPOLY):
                V.smoother = Cheb(V, self.coarse_steps if l == self.L - 1 else self.steps, lmax, ratio, pad=kind == MGPOLY)
            else:
                V.smoother = Sweeps(V)
        for V, C, T in zip(self.lev, self.lev[1:], transfers):
            V.transfer = Injection(V, T, C) if kind == MG else FullWeighting(V, T[0], T[1], C)
        self.n, self.dinv = self.lev[0].n, self.lev[0].dinv

    def cycle(self, l, r):
        V = self.lev[l]
        z, aux = V.smoother.pre(r)
        if V.transfer is None:
            return z, aux
        rc = V.transfer.restrict(V, r, z)
        zc = self.cycle(l + 1, rc)[0]
        V.transfer.prolong(z, zc)
        return V.smoother.post(r, z)

    def apply(self, r, dinv=None):
        """(z, aux) = V(0, r) in level 0's device order; aux is level 0's last t (Sweeps) or d (Cheb).  dinv: what `solve` hands
        every preconditioner; level 0 already holds it"""
        with np.errstate(all="ignore"):
            return self.cycle(0, np.asarray(r, dtype=np.float64))

    def probe(self, l, r, z, zc):
        """steps 3 and 5 on level l alone, device order: (d, rc, z after prolonging zc)"""
        V = self.lev[l]
        with np.errstate(all="ignore"):
            d = V.smoother.residual(np.asarray(r, dtype=np.float64), z)
            return d, V.transfer.weigh(d), V.transfer.prolong(np.array(z, dtype=np.float64), zc)

    def probe_w(self, l, r, w, z, zc):
        """the same behind a given w = A z, as the Chebyshev cycle's kernels take it: (rc, z after prolonging zc)"""
        T = self.lev[l].transfer
        with np.errstate(all="ignore"):
            return T.weigh(np.asarray(r, dtype=np.float64) - np.asarray(w, dtype=np.float64)), \
                T.prolong(np.array(z, dtype=np.float64), zc)

    def launches(self):
        """of one cycle: per level but the last the pre-smoothing, the transfer's own and the post-smoothing; the last level's pre"""
        return sum(sum(V.smoother.launches()) + V.transfer.launches for V in self.lev[:-1]) + self.lev[-1].smoother.launches()[0]

    def launches_per_body(self, fused_dot=True):
        """the Chebyshev kinds': p update | SpMV (+ dot pass) | alpha | the cycle | beta"""
        assert self.kind in (POLY, MGPOLY)
        return (4 if fused_dot else 5) + self.launches()

    def bytes(self):
        """the byte model of one cycle of the Chebyshev kinds, counted operation by operation"""
        assert self.kind in (POLY, MGPOLY)
        b = 0.0
        for V in self.lev:
            n, steps = float(V.n), V.smoother.steps
            b += 24.0 * n  # step 1: r, dinv in; d, z out (d = z: counted as the polynomial handle counts it)
            b += (steps - 1) * (V.spmv_bytes() + 56.0 * n)  # steps 2 .. of the pre-smoothing
            if V.transfer is None:
                break
            nc = V.transfer.nc
            b += V.spmv_bytes()  # w = A z
            b += V.transfer.bytes() + 2 * 8.0 * n + 8.0 * nc  # P^T: r and w gathered, rc out
            b += 8.0 * nc + 16.0 * n  # P: zc gathered, z in and out
            b += V.spmv_bytes() + 48.0 * n  # the post-smoothing's step 1
            b += (steps - 1) * (V.spmv_bytes() + 56.0 * n)
        return b

    def free(self):
        for V in self.lev:
            V.g.free()


class TwoSweeps:
    """the cycle of one level with its coarse levels taken away: pre, then post from that guess.  What the hierarchy adds is
    measured against it"""

    def __init__(self, V):
        self.V, self.n = V, V.n

    def apply(self, r, dinv=None):
        with np.errstate(all="ignore"):
            r = np.asarray(r, dtype=np.float64)
            return self.V.smoother.post(r, self.V.smoother.pre(r)[0])


def sgs(g, op):
    return Hierarchy(SGS, [(g, op)])


def poly(g, op, steps=None, lmax=None, ratio=None):
    return Hierarchy(POLY, [(g, op)], steps=steps, lmax=lmax, ratio=ratio)


def solve(op, plan, b_orig, dinv_orig, itermax, eps, keep_x=False):
    """pcg_ref.solve with z = r * dinv replaced by plan.apply, in the prologue and in every body: k, rr, rz, pAp, x (original
    row order); keep_x: also `xs`, the iterate after every body"""
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


# ---- the geometry and the cases

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


def trilinear(dims):
    """(ptr, col, val) of the trilinear prolongation onto an nx x ny x nz grid (all even) from the halved one, x fastest: per
    dimension an even index i takes coarse i / 2 with weight 1, an odd one (i - 1) / 2 and (i + 1) / 2 with 1/2 each, the second
    dropped where it equals the coarse dimension; a row's entries in ascending coarse number"""
    nx, ny, nz = dims
    if nx % 2 or ny % 2 or nz % 2:
        raise ValueError("odd dimension")
    cx, cy = nx // 2, ny // 2

    def line(i, nc):
        if i % 2 == 0:
            return [(i // 2, 1.0)]
        return [(j, 0.5) for j in ((i - 1) // 2, (i + 1) // 2) if j < nc]

    ptr, col, val = [0], [], []
    for z in range(nz):
        lz = line(z, nz // 2)
        for y in range(ny):
            ly = line(y, cy)
            for x in range(nx):
                for kz, wz in lz:
                    for ky, wy in ly:
                        for kx, wx in line(x, cx):
                            col.append((kz * cy + ky) * cx + kx)
                            val.append(wz * wy * wx)
                ptr.append(len(col))
    return np.array(ptr, dtype=np.int64), np.array(col, dtype=np.int64), np.array(val)


def dims_of(matrix):
    return (matrix[1],) * 3 if matrix[0] == "hpcg" else tuple(matrix[1:])


def case_transfers(kind, c):
    """the transfers of a case dict as the C API and hostapi take them, original numbering: f2c arrays (mg) or (P, omega) pairs.
    `coarse` lists them per level, an f2c ("geo", nx, ny, nz) or a P ("tri", nx, ny, nz) standing for that grid's; without it the
    geometric hierarchy of `levels` (None: auto), omega the kind's, or 1.0 on the Galerkin hierarchy"""
    if kind in (SGS, POLY):
        return []
    if c.get("coarse") is not None:
        if kind == MG:
            return [geometric_f2c(f2c[1:]) if isinstance(f2c, tuple) else np.asarray(f2c) for _, f2c in c["coarse"]]
        return [(trilinear(P[1:]) if isinstance(P[0], str) else P, omega) for _, P, omega in c["coarse"]]
    dims, out = dims_of(c["matrix"]), []
    for _ in range(geometric_levels(dims, c.get("levels")) - 1):
        out.append(geometric_f2c(dims) if kind == MG else (trilinear(dims), 1.0 if c.get("galerkin") else OMEGA[kind]))
        dims = tuple(d // 2 for d in dims)
    return out


def galerkin_gmatrix(A, P):
    """(GMatrix, scipy CSR) of P^T A P with sorted columns and exact zeros dropped"""
    Ac = (P.T.tocsr() @ A @ P).tocsr()
    Ac.sum_duplicates()
    Ac.eliminate_zeros()
    Ac.sort_indices()
    g = po.GMatrix.from_csr(Ac.indptr.astype(np.uint32), Ac.indices.astype(np.uint32), Ac.data.astype(np.float64), nc=Ac.shape[1])
    return g, Ac


def build_hierarchy(kind, c, tmpdir=None):
    """(Hierarchy, transfers) of a case dict of the kind's *_cases module.  The coarse matrices are `coarse`'s, or on a generated
    matrix the stencil regenerated on every halved grid, or with `galerkin` A_{l+1} = P_l^T A_l P_l; `steps`, `coarse_steps`,
    `lmax`, `ratio` optional (the Chebyshev kinds')"""
    g = gmatrix(c["matrix"], tmpdir)
    fmt = (c["fmt"], c["C"], c["sigma"])
    transfers = case_transfers(kind, c)
    if c.get("coarse") is not None:
        gs = [gmatrix(t[0], tmpdir) for t in c["coarse"]]
    elif c.get("galerkin"):
        import scipy.sparse as sp
        A, gs = csr(g), []
        for (ptr, col, val), _ in transfers:
            gc, A = galerkin_gmatrix(A, sp.csr_matrix((val, col, ptr), shape=(A.shape[0], A.shape[0] // 8)))
            gs.append(gc)
    else:
        dims, gs = dims_of(c["matrix"]), []
        for _ in transfers:
            dims = tuple(d // 2 for d in dims)
            gs.append(gmatrix(("dims",) + dims, tmpdir))
    levels = [(gl, operator(gl, *fmt)) for gl in [g] + gs]
    return Hierarchy(kind, levels, transfers, c.get("steps"), c.get("coarse_steps"), c.get("lmax"), c.get("ratio"), fmt), transfers


def build_case(kind, c, tmpdir=None):
    """(hierarchy, transfers, operator of level 0, b, dinv, eps); b and dinv in original row order"""
    hier, transfers = build_hierarchy(kind, c, tmpdir)
    g, op = hier.lev[0].g, hier.lev[0].op
    b = g.rhs()
    eps = c["eps_rel"] * math.sqrt(po.ddot_tree(op.to_dev(b), op.to_dev(b)))
    return hier, transfers, op, b, pcg_ref.jacobi(g), eps


def run_case(kind, c, tmpdir=None):
    hier, transfers, op, b, dinv, eps = build_case(kind, c, tmpdir)
    out = solve(op, hier, b, dinv, c["itermax"], eps)
    out["eps"], out["dinv"] = eps, dinv
    sm = [V.smoother for V in hier.lev]
    if kind == SGS:
        out["nC"] = sm[0].nC
    elif kind == POLY:
        out["coeffs"] = coeff_array(sm[0].c)
    else:
        out["L"], out["rows"] = hier.L, [V.n for V in hier.lev]
    if kind in (MG, MGFW):
        out["nC"] = [s.nC for s in sm]
    if kind == MGPOLY:
        out["coeffs"], out["intervals"] = [coeff_array(s.c) for s in sm], [(s.c["lmin"], s.c["lmax"]) for s in sm]
        out["launches"], out["bytes"] = hier.launches_per_body(), hier.bytes()
    hier.free()
    return out


def count_table(n):
    """k to eps = 1e-10 ||b|| on the n^3 stencil in CRS order at the deepest hierarchy, ratio 4: Jacobi, the polynomial (3, 16), and
    for steps 1, 2, 3 the regenerated hierarchy at omega = 0.5 and 0.25 and the Galerkin one (DESIGN 4.16's table)"""
    base = dict(matrix=("hpcg", n), fmt="crs", C=64, sigma=1, itermax=300, eps_rel=1e-10)
    g, op, b, dinv, eps = pcg_ref.build_case(dict(base, dinv="jacobi"))
    row = {"jacobi": int(pcg_ref.solve(op, b, dinv, 300, eps)["k"]),
           "poly_3_16": int(solve(op, poly(g, op, 3, None, 16.0), b, dinv, 300, eps)["k"])}
    g.free()
    L = geometric_levels((n, n, n), None)
    half, dims = [], (n, n, n)
    for _ in range(L - 1):  # the regenerated hierarchy spelled out, to carry omega = 0.5
        half.append((("dims",) + tuple(d // 2 for d in dims), ("tri",) + dims, 0.5))
        dims = tuple(d // 2 for d in dims)
    for name, kw in (("regenerated_omega_0.5", dict(coarse=half)), ("regenerated_omega_0.25", dict(levels=None)),
                     ("galerkin", dict(levels=None, galerkin=True))):
        row[name] = []
        for steps in (1, 2, 3):
            hier, transfers, op, b, dinv, eps = build_case(MGPOLY, dict(base, steps=steps, **kw))
            row[name].append(int(solve(op, hier, b, dinv, 300, eps)["k"]))
            hier.free()
    return row


def dense_apply(plan):
    """the matrix of the apply, column by column (small n)"""
    n = plan.n
    M = np.zeros((n, n))
    for i in range(n):
        e = np.zeros(n)
        e[i] = 1.0
        M[:, i] = plan.apply(e)[0]
    return M


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
