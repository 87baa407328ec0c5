"""The numerical contract of the smoothed-aggregation prolongation restated on the CPU in numpy.  TEST
INFRASTRUCTURE ONLY.  Original numbering on every side; every floating-point operation is rounded on its own (numpy's elementwise
double arithmetic; `np.add.at` adds one term at a time in the order given).  A = (ptr, col, val) is the matrix as the device stores
its rows: the GMatrix's order, which CRS and every Sell-C-sigma keep.

  d_i        the sum, in storage order from +0.0, of row i's stored entries whose column is i (sb_matrix_diagonal's)
  strong     a stored (i, j, a) with j != i, a != 0.0 and a*a > (theta*theta) * (|d_i| * |d_j|); NaN compares false; the directed
             graph as stored; a row without a strong entry is isolated
  key_i      (uint64(fmix32((i + 1) * 0x9E3779B1) >> 2) << 32) | i, the state in bits 62-63: in 2, undecided 1; out / isolated: 0
  round      m1 = max over the row and its strong entries of key, m2 the same of m1; undecided and m2 == key: in; undecided and
             m2 in state in: out; until nothing is undecided; `rounds` counts them
  aggregates roots in ascending row; pass 1: the root with the largest row among the strong entries; pass 2: the largest pass-1
             aggregate among them; isolated rows -1
  P          T[i, agg_i] = 1.0; W = A T as galerkin_ref's T (storage order, a == 0.0 skipped); P[i, J] = t - (W[i, J] * dinv_i) * s,
             t = 1.0 at J == agg_i and +0.0 elsewhere, dinv = 1.0 / d, s = omega_s / lmax, lmax the row-sum bound of DESIGN 4.15

tests/test_aggregation_ref.py pins this against properties it does not use and against scipy before anything on the GPU is
compared with it."""
import math

import numpy as np

IN, UNDECIDED, STATE = np.uint64(2 << 62), np.uint64(1 << 62), np.uint64(3 << 62)
OMEGA_S = 4.0 / 3.0
COARSEST = 64  # a level of at most this many rows is the last
DEPTH = 4


def fmix32(h):
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def keys(n):
    """the keys without their state"""
    i = np.arange(n, dtype=np.uint32)
    with np.errstate(over="ignore"):
        h = fmix32((i + np.uint32(1)) * np.uint32(0x9E3779B1))
    return ((h >> np.uint32(2)).astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)


def arrays(A):
    ptr, col, val = A
    return np.asarray(ptr).astype(np.int64), np.asarray(col).astype(np.int64), np.asarray(val, dtype=np.float64)


def diagonal(A):
    ptr, col, val = arrays(A)
    n = len(ptr) - 1
    row = np.repeat(np.arange(n), np.diff(ptr))
    d = np.zeros(n)
    on = col == row
    with np.errstate(all="ignore"):
        np.add.at(d, row[on], val[on])
    return d


def strong_graph(A, theta=0.0):
    """(sptr, scol): every row's strong columns in storage order"""
    ptr, col, val = arrays(A)
    n = len(ptr) - 1
    row = np.repeat(np.arange(n), np.diff(ptr))
    ad = np.abs(diagonal(A))
    theta2 = np.float64(theta) * np.float64(theta)
    with np.errstate(all="ignore"):
        keep = (col != row) & (val != 0.0) & (val * val > theta2 * (ad[row] * ad[col]))
    sptr = np.concatenate(([0], np.cumsum(np.bincount(row[keep], minlength=n)))).astype(np.int64)
    return sptr, col[keep]


def _nbr_max(v, sptr, scol):
    out = v.copy()
    full = np.nonzero(np.diff(sptr) > 0)[0]
    if len(full):
        out[full] = np.maximum(out[full], np.maximum.reduceat(v[scol], sptr[full]))
    return out


def mis2(sptr, scol):
    """(final keys, rounds, [rows still undecided after each round])"""
    n = len(sptr) - 1
    key = np.where(np.diff(sptr) > 0, keys(n) | UNDECIDED, np.uint64(0))
    rounds, left = 0, []
    while np.any((key & STATE) == UNDECIDED):
        m2 = _nbr_max(_nbr_max(key, sptr, scol), sptr, scol)
        und = (key & STATE) == UNDECIDED
        to_in = und & (m2 == key)
        to_out = und & ~to_in & ((m2 & STATE) == IN)
        key = key.copy()
        key[to_in] = (key[to_in] & ~STATE) | IN
        key[to_out] = np.uint64(0)
        rounds += 1
        left.append(int(np.count_nonzero((key & STATE) == UNDECIDED)))
    return key, rounds, left


def _join(a, sptr, scol):
    """a row without an aggregate takes the largest one among its strong entries"""
    best = np.full(len(a), -1, dtype=np.int64)
    full = np.nonzero(np.diff(sptr) > 0)[0]
    if len(full):
        best[full] = np.maximum.reduceat(a[scol], sptr[full])
    return np.where(a >= 0, a, best)


def aggregate(A, theta=0.0, info=False):
    """(agg int32, n_agg, rounds); info=True adds dict(left, roots, sptr, scol)"""
    sptr, scol = strong_graph(A, theta)
    key, rounds, left = mis2(sptr, scol)
    root = (key & STATE) == IN
    num = np.where(root, np.cumsum(root) - 1, -1).astype(np.int64)
    agg = _join(_join(num, sptr, scol), sptr, scol)
    isolated = np.diff(sptr) == 0
    assert np.all((agg >= 0) != isolated), "a row with strong entries found no aggregate within two hops"
    out = (agg.astype(np.int32), int(root.sum()), rounds)
    return out + (dict(left=left, roots=np.nonzero(root)[0], sptr=sptr, scol=scol),) if info else out


def tentative(agg):
    agg = np.asarray(agg).astype(np.int64)
    has = agg >= 0
    return (np.concatenate(([0], np.cumsum(has))).astype(np.uint64), agg[has].astype(np.uint32), np.ones(int(has.sum())))


def rowbound_lmax(A):
    """the largest g_i, g_i the sum from +0.0 in storage order over row i's stored entries of (|a| * sd_i) * sd[col],
    sd = sqrt(1.0 / d)"""
    ptr, col, val = arrays(A)
    n = len(ptr) - 1
    row = np.repeat(np.arange(n), np.diff(ptr))
    with np.errstate(all="ignore"):
        sd = np.sqrt(1.0 / diagonal(A))
        g = np.zeros(n)
        np.add.at(g, row, (np.abs(val) * sd[row]) * sd[col])
    if not np.all((g > 0.0) & np.isfinite(g)):
        raise ValueError("the row-sum bound is not finite and positive")
    return float(g.max())


def product_at(A, agg):
    """W = A T: ((ptr, col, val), per entry the number of terms and the sum of their magnitudes)"""
    ptr, col, val = arrays(A)
    n = len(ptr) - 1
    agg = np.asarray(agg).astype(np.int64)
    row = np.repeat(np.arange(n), np.diff(ptr))
    J = agg[col]
    on = (val != 0.0) & (J >= 0)
    nc = int(agg.max()) + 1
    pair = row[on] * nc + J[on]
    uniq, where = np.unique(pair, return_inverse=True)
    w, mag = np.zeros(len(uniq)), np.zeros(len(uniq))
    with np.errstate(all="ignore"):
        np.add.at(w, where, val[on] * 1.0)
        np.add.at(mag, where, np.abs(val[on]))
    terms = np.bincount(where, minlength=len(uniq))
    wptr = np.concatenate(([0], np.cumsum(np.bincount(uniq // nc, minlength=n))))
    return (wptr.astype(np.uint64), (uniq % nc).astype(np.uint32), w), terms, mag


def prolongation(A, theta=0.0, omega_s=OMEGA_S, lmax=None, info=False):
    """((ptr uint64, col uint32, val float64) of P, n_agg, rounds)"""
    out = aggregate(A, theta, info=info)
    agg, n_agg, rounds = out[:3]
    if n_agg == 0:
        raise ValueError("no root: every row is isolated")
    if omega_s == 0.0:
        return (tentative(agg), n_agg, rounds) + out[3:]
    if lmax is None or not lmax > 0.0:
        lmax = rowbound_lmax(A)
    s = np.float64(float(omega_s) / float(lmax))
    (wptr, wcol, w), _, _ = product_at(A, agg)
    n = len(wptr) - 1
    row = np.repeat(np.arange(n), np.diff(wptr.astype(np.int64)))
    with np.errstate(all="ignore"):
        dinv = 1.0 / diagonal(A)
        t = np.where(wcol.astype(np.int64) == agg.astype(np.int64)[row], 1.0, 0.0)
        val = t - (w * dinv[row]) * s
    return ((wptr, wcol, val), n_agg, rounds) + out[3:]


def hierarchy(A, levels=None, theta=0.0, omega_s=OMEGA_S):
    """[A_0, A_1, ...] as (ptr, col, val) in GMatrix order, [(P_l, n_agg_l, rounds_l), ...]: A_{l+1} = P_l^T A_l P_l by
    galerkin_ref.product, until `levels` levels (None: 4) or a level of at most 64 rows.  ValueError names a level that coarsens
    by less than 2 or has no root"""
    import galerkin_ref as gr
    levels = DEPTH if levels is None else levels
    mats, steps = [A], []
    while len(mats) < levels and len(mats[-1][0]) - 1 > COARSEST:
        n = len(mats[-1][0]) - 1
        try:
            P, n_agg, rounds = prolongation(mats[-1], theta, omega_s)
        except ValueError as e:
            raise ValueError("level %d: %s" % (len(mats) - 1, e))
        if 2 * n_agg > n:
            raise ValueError("level %d: %d aggregates of %d rows: coarsens by less than 2" % (len(mats) - 1, n_agg, n))
        Ac = gr.product(mats[-1], P, n_agg)[0]
        steps.append((P, n_agg, rounds))
        mats.append(Ac)
    return mats, steps


def csr_of(g):
    """(ptr, col, val) of an oracle GMatrix"""
    return g.rowPtr.astype(np.uint64), g.col.astype(np.uint32), g.val.astype(np.float64)


def build(g, fmt=("crs", 64, 1), levels=None, theta=0.0, omega_s=OMEGA_S, steps=None, found=None):
    """(precond_ref.Hierarchy of kind mgpoly on the aggregation hierarchy of GMatrix g, operator of level 0, b, eps = 1e-10 ||b||,
    (mats, steps)); found: that pair where it has been made already"""
    from oracle import pyoracle as po

    import pcg_ref
    import precond_ref as mp
    mats, st = found if found is not None else hierarchy(csr_of(g), levels, theta, omega_s)
    gs = [g] + [po.GMatrix.from_csr(M[0].astype(np.uint32), M[1], M[2], nc=len(M[0]) - 1) for M in mats[1:]]
    lev = [(q, pcg_ref.operator(q, *fmt)) for q in gs]
    hier = mp.Hierarchy(mp.MGPOLY, lev, [(P, 1.0) for P, _, _ in st], steps=steps, fmt=fmt)
    op, b = lev[0][1], g.rhs()
    eps = 1e-10 * math.sqrt(po.ddot_tree(op.to_dev(b), op.to_dev(b)))
    return hier, op, b, eps, (mats, st)


# ---- the hand-made matrices of the GPU tests: (ptr, col, val) with ascending columns, and theta

def chain(n=10):
    """tridiagonal (-1, 2, -1): many rounds on few rows"""
    ptr, col, val = [0], [], []
    for i in range(n):
        for j in (i - 1, i, i + 1):
            if 0 <= j < n:
                col.append(j), val.append(2.0 if j == i else -1.0)
        ptr.append(len(col))
    return (np.array(ptr, np.uint64), np.array(col, np.uint32), np.array(val)), 0.0


def threshold():
    """theta = 0.5, d = 4 everywhere: |a| = 2 sits exactly at the threshold and is NOT strong, 2.5 is; row 5 keeps only a stored
    0.0 and an entry at the threshold and is isolated; row 6 is a bare diagonal"""
    rows = {0: {0: 4.0, 1: -2.5, 2: -2.0}, 1: {0: -2.5, 1: 4.0, 3: 2.5}, 2: {0: -2.0, 2: 4.0, 3: -3.0, 4: 0.0},
            3: {1: 2.5, 2: -3.0, 3: 4.0}, 4: {2: 0.0, 4: 4.0, 5: -2.0, 3: 2.25}, 5: {4: -2.0, 5: 4.0, 0: 0.0}, 6: {6: 4.0}}
    return _from_rows(rows, 7), 0.5


def one_way():
    """structurally non-symmetric: rows 4 and 5 reach the rest only along their own out-edges, nothing points back at them"""
    rows = {0: {0: 3.0, 1: -1.0}, 1: {0: -1.0, 1: 3.0, 2: -1.0}, 2: {1: -1.0, 2: 3.0, 3: -1.0}, 3: {2: -1.0, 3: 3.0},
            4: {4: 3.0, 3: -1.0}, 5: {5: 3.0, 4: -2.0}, 6: {6: 3.0, 5: -1.0, 0: -1.0}}
    return _from_rows(rows, 7), 0.0


def with_nan():
    """a NaN off the diagonal is never strong (and poisons no decision); the NaN reaches W and P"""
    (ptr, col, val), _ = chain(8)
    val = val.copy()
    val[int(ptr[3]) + 2] = np.nan  # A[3, 4]
    return (ptr, col, val), 0.0


def all_isolated(n=5):
    return (np.arange(n + 1, dtype=np.uint64), np.arange(n, dtype=np.uint32), np.full(n, 2.0)), 0.0


def arrow(n=130):
    """rows 1 .. n-1 hold their diagonal and one entry in column 0; row 0 its diagonal alone: every row but the first is a root"""
    rows = {i: ({0: -1.0, i: 4.0} if i else {0: 4.0}) for i in range(n)}
    return _from_rows(rows, n), 0.0


def _from_rows(rows, n):
    ptr, col, val = [0], [], []
    for i in range(n):
        for j in sorted(rows[i]):
            col.append(j), val.append(rows[i][j])
        ptr.append(len(col))
    return np.array(ptr, np.uint64), np.array(col, np.uint32), np.array(val, dtype=np.float64)


HAND_MADE = {"chain10": chain, "threshold": threshold, "one_way": one_way, "nan": with_nan}
GRIDS = [(2, 2, 2), (6, 4, 2), (8, 4, 4), (10, 4, 2), (12, 8, 20), (34, 6, 10)]
FORMATS = {"crs": ("crs", 64, 1), "sell_64_1": ("scs", 64, 1), "sell_64_256": ("scs", 64, 256), "sell_4_8": ("scs", 4, 8)}


def digest(P):
    import galerkin_ref as gr
    return gr.digest(P)
