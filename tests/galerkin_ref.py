"""The numerical contract of the Galerkin product A_c = P^T A P restated on the CPU in plain Python and numpy.
TEST INFRASTRUCTURE ONLY.  Original numbering on every side; every operation is rounded on its own (a Python float is a double,
and `a * w` then `s + t` are one multiply and one addition).

  T[i, J]:    s = +0.0 ; the entries e of row i of A in the order the row is stored (the GMatrix's order, which CRS and every
              Sell-C-sigma keep) whose value does not compare equal to 0.0 ; inside each the entries q of row col_e of P in storage
              order whose weight is not 0.0 ; for col_q == J:  t = a_e * p_q ; s = s + t.  T has the entry where a term exists.
  A_c[I, J]:  s = +0.0 ; the entries (i, w) of row I of P^T with w != 0.0 in ascending fine row i (equal rows: storage order) ;
              where T[i, J] exists:  u = w * T[i, J] ; s = s + u.  A sum that compares equal to 0.0 is dropped, NaN is kept;
              columns ascending, 64-bit row pointers.

tests/test_galerkin_host.py pins this against scipy before anything on the GPU is compared with it."""
import numpy as np


def _lists(M):
    ptr, col, val = M
    return (np.asarray(ptr).astype(np.int64).tolist(), np.asarray(col).astype(np.int64).tolist(),
            np.asarray(val, dtype=np.float64).tolist())


def product(A, P, nc, terms=False):
    """A, P: (ptr, col, val) CSR triples, P of len(A rows) x nc.  Returns ((ptr uint64, col uint32, val float64) of A_c, the
    number of entries dropped as 0.0, (the most distinct columns of a row of T, of a row of P^T T before the drop)); terms=True
    adds a dict (I, J) -> (m, sum |w * a * p|) over the KEPT entries: the term count and the magnitude of the bound"""
    aptr, acol, aval = _lists(A)
    pptr, pcol, pval = _lists(P)
    n = len(aptr) - 1
    assert len(pptr) == n + 1
    T, mag, cnt = [], [], []
    for i in range(n):
        acc, am, ac = {}, {}, {}
        for e in range(aptr[i], aptr[i + 1]):
            a = aval[e]
            if a == 0.0:
                continue
            c = acol[e]
            for q in range(pptr[c], pptr[c + 1]):
                w = pval[q]
                if w == 0.0:
                    continue
                J = pcol[q]
                t = a * w
                acc[J] = acc.get(J, 0.0) + t
                if terms:
                    am[J] = am.get(J, 0.0) + abs(t)
                    ac[J] = ac.get(J, 0) + 1
        T.append(acc), mag.append(am), cnt.append(ac)
    rows = [[] for _ in range(nc)]
    for i in range(n):
        for q in range(pptr[i], pptr[i + 1]):
            if pval[q] != 0.0:
                rows[pcol[q]].append((i, pval[q]))
    ptr, col, val, dropped, max_ac, info = [0], [], [], 0, 0, {}
    for I in range(nc):
        acc, am, ac = {}, {}, {}
        for i, w in rows[I]:
            for J, tv in T[i].items():
                u = w * tv
                acc[J] = acc.get(J, 0.0) + u
                if terms:
                    am[J] = am.get(J, 0.0) + abs(w) * mag[i][J]
                    ac[J] = ac.get(J, 0) + cnt[i][J]
        max_ac = max(max_ac, len(acc))
        for J in sorted(acc):
            if acc[J] == 0.0:
                dropped += 1
                continue
            col.append(J), val.append(acc[J])
            if terms:
                info[(I, J)] = (ac[J], am[J])
        ptr.append(len(col))
    out = (np.array(ptr, dtype=np.uint64), np.array(col, dtype=np.uint32), np.array(val, dtype=np.float64))
    maxima = (max([len(t) for t in T] + [0]), max_ac)
    return (out, dropped, maxima, info) if terms else (out, dropped, maxima)


def same_csr(got, want, what=""):
    """bit for bit: pointers, columns and the values' bytes (NaN equal to NaN with the same payload)"""
    for name, a, b, dt in zip(("ptr", "col", "val"), got, want, (np.uint64, np.uint32, np.float64)):
        a, b = np.ascontiguousarray(a, dtype=dt), np.ascontiguousarray(b, dtype=dt)
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        bad = np.nonzero(a.view(np.uint64 if dt == np.float64 else dt) != b.view(np.uint64 if dt == np.float64 else dt))[0]
        assert bad.size == 0, (what, name, "first difference at", int(bad[0]), a[bad[0]], b[bad[0]], "of", bad.size)


def scipy_product(A, P, nc):
    """hostapi.mg_galerkin's: (P^T A P) in CSR, duplicates summed, exact zeros dropped, columns sorted"""
    import scipy.sparse as sp
    n = len(A[0]) - 1
    As = sp.csr_matrix((np.asarray(A[2], dtype=np.float64), np.asarray(A[1]).astype(np.int64), np.asarray(A[0]).astype(np.int64)), shape=(n, n))
    Ps = sp.csr_matrix((np.asarray(P[2], dtype=np.float64), np.asarray(P[1]).astype(np.int64), np.asarray(P[0]).astype(np.int64)), shape=(n, nc))
    Ac = (Ps.T.tocsr() @ As @ Ps).tocsr()
    Ac.sum_duplicates()
    Ac.eliminate_zeros()
    Ac.sort_indices()
    return Ac.indptr.astype(np.uint64), Ac.indices.astype(np.uint32), Ac.data.astype(np.float64)


def scaled_hpcg8():
    """D^1/2 A D^1/2 of the 8^3 stencil, d_i = 1 + (i mod 7) / 3: a matrix whose products are not exact.  (ptr, col, val) with the
    generator's row order; every operation numpy's own rounded double arithmetic"""
    from sparsebench_amd import hostapi
    p = hostapi.Problem("generate", 8, 8, 8, fmt="crs", upload=False)
    ptr, (col, val) = p.array("rowPtr").astype(np.uint64), p.gm_entries()
    p.free()
    d = np.sqrt(1.0 + (np.arange(512) % 7) / 3.0)
    rows = np.repeat(np.arange(512), np.diff(ptr.astype(np.int64)))
    val = (d[rows] * val.astype(np.float64)) * d[col]
    return ptr, col.copy(), val


def cancelling():
    """a 4 x 4 matrix and a 4 x 2 P with weights +1 and -1 that cancel exactly in A_c[0, 1] and A_c[1, 0]; the rest is kept"""
    A = (np.array([0, 1, 2, 3, 4], dtype=np.uint64), np.array([0, 1, 2, 3], dtype=np.uint32), np.array([2.0, 2.0, 3.0, 5.0]))
    P = (np.array([0, 2, 4, 5, 6], dtype=np.uint64), np.array([0, 1, 0, 1, 0, 1], dtype=np.uint32),
         np.array([1.0, 1.0, 1.0, -1.0, 1.0, 1.0]))
    return A, P, 2


def underflowing():
    """diag(2, 2, 3, 5) scaled by 2^-540 and a P whose second column is reached through weights of 2^-540 alone: those products
    underflow to 0.0, T keeps the entries, A_c[1, 1] sums to 0.0 and is dropped; A_c[0, 0] is kept"""
    s = 2.0 ** -540
    A = (np.array([0, 1, 2, 3, 4], dtype=np.uint64), np.array([0, 1, 2, 3], dtype=np.uint32), np.array([2.0, 2.0, 3.0, 5.0]) * s)
    P = (np.array([0, 1, 2, 3, 4], dtype=np.uint64), np.array([0, 0, 1, 1], dtype=np.uint32), np.array([1.0, 0.5, s, s]))
    return A, P, 2


def scaled_case(fmt=("crs", 64, 1), steps=2):
    """the two-level solve on the scaled 8^3 matrix with the trilinear P, omega = 1.0 and THIS file's coarse operator:
    (precond_ref.Hierarchy, operator of level 0, b, eps, (A, P, A_c)); b = 1, eps = 1e-10 ||b||"""
    import math

    from oracle import pyoracle as po

    import pcg_ref
    import precond_ref as mp
    A, P = scaled_hpcg8(), mp.trilinear((8, 8, 8))
    Ac = product(A, P, 64)[0]
    gs = [po.GMatrix.from_csr(M[0].astype(np.uint32), M[1], M[2]) for M in (A, Ac)]
    levels = [(g, pcg_ref.operator(g, *fmt)) for g in gs]
    hier = mp.Hierarchy(mp.MGPOLY, levels, [(P, 1.0)], steps=steps, fmt=fmt)
    op, b = levels[0][1], gs[0].rhs()
    eps = 1e-10 * math.sqrt(po.ddot_tree(op.to_dev(b), op.to_dev(b)))
    return hier, op, b, eps, (A, P, Ac)


def digest(M):
    """nnz and a SHA-256 over the bytes of ptr (uint64), col (uint32), val (float64)"""
    import hashlib
    h = hashlib.sha256()
    for a, dt in zip(M, (np.uint64, np.uint32, np.float64)):
        h.update(np.ascontiguousarray(a, dtype=dt).tobytes())
    return {"nnz": int(len(M[1])), "sha256": h.hexdigest()}


def stencil(dims):
    """(ptr, col, val) of the generator's 27-point stencil on a grid, the generator's row order"""
    from sparsebench_amd import hostapi
    p = hostapi.Problem("generate", *dims, fmt="crs", upload=False)
    A = (p.array("rowPtr").astype(np.uint64), *p.gm_entries())
    p.free()
    return A


def hierarchy(dims, levels):
    """[(A_c, dropped, maxima), ...] of levels 1 .. levels - 1 on the stencil with the repository's trilinear P"""
    from sparsebench_amd import hostapi
    A, out = stencil(dims), []
    for _ in range(levels - 1):
        P = hostapi.mg_trilinear(*dims)
        dims = tuple(d // 2 for d in dims)
        out.append(product(A, P, dims[0] * dims[1] * dims[2]))
        A = out[-1][0]
    return out


GOLDEN_PRODUCTS = {"hpcg8_L3": ((8, 8, 8), 3), "hpcg16_L4": ((16, 16, 16), 4), "dims_12_8_20_L3": ((12, 8, 20), 3)}
