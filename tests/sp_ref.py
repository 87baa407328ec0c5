"""fp32 restatement of the single-precision hot path, for the tests only (numpy; the product never imports it).

Every operation is a float32 operation in the reference's order (src/matrix-CRS.c:46-60, src/matrix-SCS.c:198-228,
src/solver.c:16-62, src/CGSolver.c:63-128 of the FLOAT_TYPE=SP build): each product rounded before its add, sums in
float32.  The dot orders are DESIGN 4.3's: the tree (level 0 xor butterfly over aligned 64-element groups, level 1
((q0 + q1) + q2) + q3, level 2 over 1024 threads and 16 waves) and seq (one left-to-right chain from +0.0).
"""
import numpy as np

F = np.float32


def _f(a):
    return np.ascontiguousarray(a, dtype=F)


def spmv_crs(rowPtr, colInd, val, x):
    """y[r] = sum over the row, left to right: acc = acc + val * x[col] (one float32 add per position)"""
    rowPtr = np.asarray(rowPtr, np.int64)
    val, x = _f(val), _f(x)
    nr = len(rowPtr) - 1
    lens = np.diff(rowPtr)
    acc = np.zeros(nr, F)
    for j in range(int(lens.max()) if nr else 0):
        rows = np.nonzero(lens > j)[0]
        k = rowPtr[rows] + j
        acc[rows] = acc[rows] + val[k] * x[np.asarray(colInd)[k]]
    return acc


def spmv_scs(chunkPtr, chunkLens, colInd, val, C, oldToNew, nr, x):
    """Sell-C-sigma from the host layout (original column numbers), padding included (column 0, value 0.0: "x[0] * 0");
    y in the caller's row order"""
    val, x = _f(val), _f(x)
    colInd = np.asarray(colInd, np.int64)
    nChunks = len(chunkLens)
    acc = np.zeros(nChunks * C, F)
    q = np.arange(nChunks * C)
    c, k = q // C, q % C
    cp, ln = np.asarray(chunkPtr, np.int64)[c], np.asarray(chunkLens, np.int64)[c]
    for j in range(int(ln.max()) if len(ln) else 0):
        m = ln > j
        idx = cp[m] + j * C + k[m]
        acc[m] = acc[m] + val[idx] * x[colInd[idx]]
    return acc[np.asarray(oldToNew, np.int64)[:nr]] if oldToNew is not None else acc[:nr]


def waxpby(alpha, x, beta, y):
    """src/solver.c:16-39, its three branches"""
    alpha, beta, x, y = F(alpha), F(beta), _f(x), _f(y)
    if alpha == F(1.0):
        return x + beta * y
    if beta == F(1.0):
        return alpha * x + y
    return alpha * x + beta * y


def _xor_sum(v, width):
    """xor butterfly over the last axis (width lanes): v = v + v[lane ^ o], o = 1, 2, 4, ..."""
    idx = np.arange(width)
    o = 1
    while o < width:
        v = v + v[..., idx ^ o]
        o <<= 1
    return v


def level0(a, b):
    """one partial per aligned 64 elements, 4 * ceil(n / 256) of them; missing elements are +0.0"""
    a, b = _f(a), _f(b)
    n = len(a)
    m = (n + 255) // 256
    t = np.zeros(m * 256, F)
    t[:n] = a * b
    return _xor_sum(t.reshape(-1, 64), 64)[:, 0].copy()


def level1(q):
    q = _f(q).reshape(-1, 4)
    return ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]


def level2(l1):
    """1024 threads: thread t adds values t, t + 1024, ... from +0.0; each wave butterflies; waves added in order"""
    l1 = _f(l1)
    s = np.zeros(1024, F)
    for i0 in range(0, len(l1), 1024):
        chunk = l1[i0:i0 + 1024]
        s[:len(chunk)] = s[:len(chunk)] + chunk
    w = _xor_sum(s.reshape(16, 64), 64)[:, 0]
    total = w[0]
    for i in range(1, 16):
        total = F(total + w[i])
    return F(total)


def dot_tree(a, b):
    return level2(level1(level0(a, b)))


def dot_seq(a, b):
    """CG_FLOAT sum = 0.0; sum += a[i] * b[i], left to right"""
    p = _f(a) * _f(b)
    return F(np.add.accumulate(np.concatenate([np.zeros(1, F), p]), dtype=F)[-1])


def normr_fails(rr, eps):
    """!(normr > eps): normr = sqrt(rtrans) in double, stored to a float (src/CGSolver.c:100,116)"""
    return not (F(np.sqrt(np.float64(rr))) > F(eps))


def cg(spmv, b, itermax, eps=0.0, dot=dot_tree):
    """solveCG of the SP build (src/CGSolver.c:62-141) over `spmv` (x -> A x in float32): (k, rr history, p.Ap history, x)"""
    b = _f(b)
    n = len(b)
    x = np.zeros(n, F)
    p = waxpby(1.0, x, 0.0, x)
    Ap = spmv(p)
    r = waxpby(1.0, b, -1.0, Ap)
    rtrans = dot(r, r)
    rr, pap = [rtrans], []
    fails = normr_fails(rtrans, eps)
    k = 1
    with np.errstate(all="ignore"):
        while k < itermax and not fails:
            if k == 1:
                p = waxpby(1.0, r, 0.0, r)
            else:
                old = rtrans
                rtrans = dot(r, r)
                rr.append(rtrans)
                beta = F(rtrans / old)  # the float division, carried by `double beta` into waxpby's CG_FLOAT beta
                p = waxpby(1.0, r, beta, p)
            fails = normr_fails(rtrans, eps)
            Ap = spmv(p)
            t = dot(p, Ap)
            pap.append(t)
            alpha = F(rtrans / t)
            x = waxpby(1.0, x, alpha, p)
            r = waxpby(1.0, r, -alpha, Ap)
            k += 1
    return k, np.array(rr, F), np.array(pap, F), x
