"""The CPU restatement of the smoothed-aggregation prolongation (tests/aggregation_ref.py) pinned independently of
itself, before anything on the GPU is compared with it: the keys against a plain-integer murmur3 finaliser; the rounds and both
join passes against a row-by-row dictionary walk of the contract's sentences; on symmetric graphs the properties of a distance-2
maximal independent set and of its aggregates, read off scipy's powers of the graph; on every graph the numbering, P against
scipy's T - s D^-1 A T, the row sums, the tentative T; the case list's two conditions; the whole solves against
tests/golden/aggregation_hist.json.

P against scipy's T - s * (D^-1 A T): |P - scipy| <= (m + 2) 2^-53 (|t| + s |dinv_i| sum |a|) per entry, m the terms of W[i, J].
Bit for bit on the unscaled stencil at theta = 0?  Against that expression it does NOT hold: 1 / 27 is not exact and
s * (dinv * w) associates differently from (w * dinv) * s, which moves last bits.  It DOES hold against scipy's
T - (D^-1 (A T)) * s, the contract's order, because every W[i, J] on the stencil is a sum of small integers, exact in any order;
both are asserted below."""
import numpy as np
import pytest

import aggregation_cases as ac
import aggregation_ref as ar
import galerkin_ref as gr
from conftest import load_json

sp = pytest.importorskip("scipy.sparse")


def fmix32_int(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def test_keys_are_murmur3s_finaliser_of_the_golden_ratio_multiple():
    n = 3000
    want = [((fmix32_int(((i + 1) * 0x9E3779B1) & 0xFFFFFFFF) >> 2) << 32) | i for i in range(n)]
    got = ar.keys(n)
    assert got.dtype == np.uint64 and got.tolist() == want
    assert len(set(want)) == n and max(want) < 1 << 62  # distinct, and the two state bits are free
    assert fmix32_int(0) == 0 and ar.fmix32(np.array([0xDEADBEEF], dtype=np.uint32))[0] == fmix32_int(0xDEADBEEF)


def walk(A, theta):
    """the contract's sentences, one row at a time on Python integers and floats: (agg, n_agg, rounds)"""
    ptr, col, val = [np.asarray(a).tolist() for a in A]
    n = len(ptr) - 1
    d = [0.0] * n
    for i in range(n):
        for e in range(ptr[i], ptr[i + 1]):
            if col[e] == i:
                d[i] = d[i] + val[e]
    nb = [[col[e] for e in range(ptr[i], ptr[i + 1])
           if col[e] != i and val[e] != 0.0 and val[e] * val[e] > (theta * theta) * (abs(d[i]) * abs(d[col[e]]))] for i in range(n)]
    IN, UND = 2 << 62, 1 << 62
    base = [((fmix32_int(((i + 1) * 0x9E3779B1) & 0xFFFFFFFF) >> 2) << 32) | i for i in range(n)]
    key = [(base[i] | UND) if nb[i] else 0 for i in range(n)]
    rounds = 0
    while any(k >> 62 == 1 for k in key):
        m1 = [max([key[i]] + [key[j] for j in nb[i]]) for i in range(n)]
        m2 = [max([m1[i]] + [m1[j] for j in nb[i]]) for i in range(n)]
        new = list(key)
        for i in range(n):
            if key[i] >> 62 == 1:
                if m2[i] == key[i]:
                    new[i] = base[i] | IN
                elif m2[i] >> 62 == 2:
                    new[i] = 0
        key, rounds = new, rounds + 1
    roots = [i for i in range(n) if key[i] >> 62 == 2]
    num = {r: a for a, r in enumerate(roots)}
    agg = [num.get(i, -1) for i in range(n)]
    one = list(agg)
    for i in range(n):
        if agg[i] < 0 and nb[i]:
            mine = [j for j in nb[i] if j in num]
            if mine:
                one[i] = num[max(mine)]
    two = list(one)
    for i in range(n):
        if one[i] < 0 and nb[i]:
            two[i] = max(one[j] for j in nb[i])
    return two, len(roots), rounds


def matrices():
    out = [("dims_%d_%d_%d" % d, gr.stencil(d), 0.0, True) for d in ar.GRIDS[:5]]
    out += [(name, *make(), name == "chain10") for name, make in ar.HAND_MADE.items()]
    out.append(("arrow", *ar.arrow(130), False))
    out.append(("scaled8", gr.scaled_hpcg8(), 0.0, True))
    out.append(("scaled8_at_the_threshold", gr.scaled_hpcg8(), 1.0 / 27.0, False))
    return out


MATRICES = matrices()


@pytest.mark.parametrize("name,A,theta,symmetric", MATRICES, ids=[m[0] for m in MATRICES])
def test_rounds_and_joins_equal_the_row_by_row_walk(name, A, theta, symmetric):
    agg, n_agg, rounds = ar.aggregate(A, theta)
    want = walk(A, theta)
    assert (agg.tolist(), n_agg, rounds) == want


def graph(A, theta):
    sptr, scol = ar.strong_graph(A, theta)
    n = len(sptr) - 1
    return sp.csr_matrix((np.ones(len(scol)), scol, sptr), shape=(n, n))


@pytest.mark.parametrize("name,A,theta,symmetric", [m for m in MATRICES if m[3]], ids=[m[0] for m in MATRICES if m[3]])
def test_on_a_symmetric_graph_the_roots_are_a_distance_2_maximal_independent_set(name, A, theta, symmetric):
    S = graph(A, theta)
    assert (S != S.T).nnz == 0
    agg, n_agg, rounds, info = ar.aggregate(A, theta, info=True)
    roots = info["roots"]
    two = (S + S @ S).tocsr()  # > 0 where a walk of one or two hops exists
    near = two[roots][:, roots].toarray() > 0
    np.fill_diagonal(near, False)
    assert not near.any()  # pairwise more than two hops apart
    isolated = np.diff(S.indptr) == 0
    assert np.array_equal(agg < 0, isolated) and np.all(agg[isolated] == -1)
    rows = np.nonzero(agg >= 0)[0]
    reach = (two + sp.identity(S.shape[0])).tocsr()
    assert np.all(np.asarray(reach[rows, roots[agg[rows]]]).ravel() > 0)  # every aggregated row within two hops of its root
    # maximal: every row that is not isolated has a root within two hops
    assert np.all(np.asarray(reach[:, roots].sum(axis=1)).ravel()[~isolated] > 0)


@pytest.mark.parametrize("name,A,theta,symmetric", MATRICES, ids=[m[0] for m in MATRICES])
def test_on_every_graph_numbering_prolongation_and_row_sums(name, A, theta, symmetric):
    agg, n_agg, rounds, info = ar.aggregate(A, theta, info=True)
    roots = info["roots"]
    assert np.all(np.diff(roots) > 0) and agg[roots].tolist() == list(range(n_agg))  # the numbers ascend with the roots' rows
    assert n_agg == len(roots) and agg.max() == n_agg - 1 and set(agg[agg >= 0].tolist()) == set(range(n_agg))
    # omega_s = 0: the 0/1 T, one entry per aggregated row
    T = ar.prolongation(A, theta, omega_s=0.0)[0]
    assert np.array_equal(np.diff(T[0].astype(np.int64)), (agg >= 0).astype(np.int64)) and set(T[2].tolist()) == {1.0}
    assert np.array_equal(T[1], agg[agg >= 0].astype(np.uint32))
    if name == "arrow":
        return  # it has a P, but nothing below depends on the graph
    lmax = ac.HAND_LMAX if name in ar.HAND_MADE else ar.rowbound_lmax(A)
    (ptr, col, val), n2, r2 = ar.prolongation(A, theta, lmax=lmax)
    assert (n2, r2) == (n_agg, rounds)
    n = len(ptr) - 1
    s = ar.OMEGA_S / lmax
    aptr, acol, aval = ar.arrays(A)
    ok = ~np.isnan(aval)
    As = sp.csr_matrix((np.where(ok, aval, 0.0), acol, aptr), shape=(n, n))
    d = ar.diagonal(A)
    Ts = sp.csr_matrix((T[2], T[1].astype(np.int64), T[0].astype(np.int64)), shape=(n, n_agg))
    want = (Ts - s * (sp.diags(1.0 / d) @ As @ Ts)).tocsr()
    (wptr, wcol, w), terms, mag = ar.product_at(A, agg)
    assert np.array_equal(wptr, ptr) and np.array_equal(wcol, col)  # P has W's pattern
    row = np.repeat(np.arange(n), np.diff(ptr.astype(np.int64)))
    assert np.all(np.diff(col.astype(np.int64))[np.diff(row) == 0] > 0)  # columns ascending
    got = np.asarray(want[row, col.astype(np.int64)]).ravel()
    t = (col.astype(np.int64) == agg[row]).astype(np.float64)
    bound = (terms + 2) * 2.0 ** -53 * (t + s * np.abs(1.0 / d)[row] * mag)
    num = ~np.isnan(val)
    assert np.all(np.abs(val - got)[num] <= bound[num]) and (name == "nan") == (not num.all())
    assert abs(want).sum() > 0 and want.nnz <= len(col)
    if name.startswith("dims_"):  # the unscaled stencil at theta = 0: bit for bit once scipy multiplies in the contract's order
        exact = (Ts - (sp.diags(1.0 / d) @ (As @ Ts)) * s).tocsr()
        assert np.array_equal(val.view(np.uint64), np.asarray(exact[row, col.astype(np.int64)]).ravel().view(np.uint64))
        assert not np.array_equal(val.view(np.uint64), got.view(np.uint64)) or n <= 8
    # P 1 = (I - s D^-1 A) 1 on the rows all of whose neighbours are aggregated
    arow = np.repeat(np.arange(n), np.diff(aptr))
    full = np.ones(n, dtype=bool)
    np.logical_and.at(full, arow, (agg[acol] >= 0) | (aval == 0.0))
    full &= ~np.isnan(np.bincount(arow, weights=aval, minlength=n))
    sums = np.bincount(row, weights=np.where(num, val, 0.0), minlength=n)
    rhs = 1.0 - s * (1.0 / d) * np.bincount(arow, weights=np.where(ok, aval, 0.0), minlength=n)
    slack = (np.diff(aptr) + 3) * 2.0 ** -52 * (1.0 + s * np.abs(1.0 / d) * np.bincount(arow, weights=np.abs(np.where(ok, aval, 0.0)), minlength=n))
    assert full.any() and np.all(np.abs(sums - rhs)[full] <= slack[full])


def test_the_case_list_meets_the_two_conditions():
    """(12, 8, 20) needs at least two levels; some grid ends with undecided rows in its last-but-one round on fewer than 64 rows"""
    mats, steps = ar.hierarchy(gr.stencil((12, 8, 20)))
    assert len(mats) >= 2 and len(mats[1][0]) - 1 <= ar.COARSEST
    lefts = {d: ar.aggregate(gr.stencil(d), info=True)[3]["left"] for d in ar.GRIDS}
    assert any(len(v) >= 2 and 0 < v[-2] < 64 for v in lefts.values()), lefts
    assert all(v[-1] == 0 for v in lefts.values())
    agg = ar.aggregate(gr.stencil((2, 2, 2)))
    assert agg[1] == 1 and set(agg[0].tolist()) == {0}


def test_hierarchy_refuses_by_name():
    with pytest.raises(ValueError, match="level 0: 129 aggregates of 130 rows: coarsens by less than 2"):
        ar.hierarchy(ar.arrow(130)[0])
    big = ar.all_isolated(100)[0]
    with pytest.raises(ValueError, match="level 0: no root"):
        ar.hierarchy(big)
    assert ar.aggregate(big)[1:] == (0, 0)


def test_golden_prolongations_are_the_restatements():
    e = load_json("aggregation_hist.json")["prolongations"]
    for dims in ar.GRIDS:
        P, n_agg, rounds, info = ar.prolongation(gr.stencil(dims), info=True)
        want = e["dims_%d_%d_%d" % dims]
        assert dict(ar.digest(P), n_agg=n_agg, rounds=rounds, left=info["left"]) == want
    for name, make in ar.HAND_MADE.items():
        A, theta = make()
        P, n_agg, rounds = ar.prolongation(A, theta, lmax=ac.HAND_LMAX)
        assert dict(ar.digest(P), n_agg=n_agg, rounds=rounds) == {k: v for k, v in e[name].items() if k != "left"}


@pytest.mark.parametrize("name", ["pcg_hpcg16_crs_steps1", "pcg_scaled8_sell_64_256_steps2", "pcg_irregular12_sell_64_256_steps2",
                                  "bicgstab_cd16_sell_64_256_steps1"])
def test_whole_solves_converge_and_are_the_golden(name):
    rec = load_json("aggregation_hist.json")["solves"][name]
    got = ac.record(name)
    assert got == rec
    assert 1 < got["k"] < ac.ITERMAX  # converged to 1e-10 ||b|| inside the budget
    assert len(got["rows"]) >= 2 and all(2 * b <= a for a, b in zip(got["rows"], got["rows"][1:]))


def test_the_table_of_iteration_counts_is_the_goldens():
    """the counts the documents quote; the 32^3 row is left to the golden's maker"""
    t = load_json("aggregation_hist.json")["table"]
    assert set(t) == set(ac.TABLE_ROWS)
    for name in ("hpcg16", "cd16_bicgstab"):
        assert ac.table_row(*ac.TABLE_ROWS[name]) == t[name]
    for row in t.values():  # the hierarchy beats Jacobi everywhere, and two steps beat one
        assert row["aggregation_steps2"] < row["aggregation_steps1"] < row["jacobi"]
