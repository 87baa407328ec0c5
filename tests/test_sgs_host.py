"""The CPU restatement of SGS-preconditioned CG (tests/precond_ref.py) pinned before the GPU is compared with it:
the colouring is proper and greedy-minimal, the apply is the two triangular solves of the colour-permuted matrix with D in
between, M is symmetric, the solve is PCG under that operator (against scipy), a diagonal matrix gives Jacobi PCG bit for bit,
the iteration count drops against Jacobi, and tests/golden/sgs_hist.json holds what the restatement gives."""
import numpy as np
import pytest

import pcg_ref
import precond_ref as ref
import sgs_cases
from conftest import load_json


@pytest.fixture(scope="module")
def golden():
    return load_json("sgs_hist.json")


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("sgs")


def plan_of(matrix, fmt="crs", C=64, sigma=1, tmp=None):
    """(g, operator, the one-level hierarchy, its Sweeps)"""
    g = pcg_ref.gmatrix(matrix, tmp)
    op = pcg_ref.operator(g, fmt, C, sigma)
    plan = ref.sgs(g, op)
    return g, op, plan, plan.lev[0].smoother


COLOURED = [(("dims", 5, 5, 5), "crs", 1), (("hpcg", 16), "crs", 1), (("dims", 7, 7, 6), "scs", 256), (("irregular", 12), "crs", 1),
            (("irregular", 12), "scs", 256), (("file", sgs_cases.BAND_KLEIN), "crs", 1)]


@pytest.mark.parametrize("matrix,fmt,sigma", COLOURED)
def test_colouring_is_proper_and_greedy_minimal(matrix, fmt, sigma):
    g, op, plan, sw = plan_of(matrix, fmt, 64, sigma)
    n, colour = sw.n, sw.colour
    adj = [set() for _ in range(n)]
    row = np.repeat(np.arange(n), np.diff(sw.kptr))
    for i, j in zip(row.tolist(), sw.kcol.tolist()):
        adj[i].add(j), adj[j].add(i)
    for i in range(n):
        assert i not in adj[i]
        around = {int(colour[j]) for j in adj[i]}
        assert int(colour[i]) not in around  # proper
        before = {int(colour[j]) for j in adj[i] if j < i}
        assert set(range(int(colour[i]))) <= before  # every smaller colour was taken by an earlier neighbour
    assert sw.nC == int(colour.max()) + 1
    if matrix in (("dims", 5, 5, 5), ("hpcg", 16)):
        assert sw.nC == 8
    if matrix == ("dims", 5, 5, 5):
        assert [len(r) for r in sw.rows] == [27, 18, 18, 12, 18, 12, 12, 8]
    g.free()


def test_hand_made_matrices_colour_as_designed(tmp):
    for kind, nC in (("one", 1), ("diagonal", 1), ("arrow", 2), ("zeros", 2)):
        g, op, plan, sw = plan_of(("file", sgs_cases.hand_made(kind, tmp)))
        assert sw.nC == nC, kind
        if kind == "arrow":
            assert len(sw.upper(0)[0]) == 299 and all(len(sw.lower(i)[0]) == 1 for i in range(1, 300))
        if kind == "zeros":
            assert len(g.val) > len(sw.kval) + g.nr  # explicit zeros are stored and were dropped
            assert max(len(sw.lower(i)[0]) + len(sw.upper(i)[0]) for i in range(g.nr)) == 2
        g.free()


@pytest.mark.parametrize("matrix,fmt,sigma", [(("dims", 5, 5, 5), "crs", 1), (("dims", 7, 7, 6), "scs", 256), (("irregular", 12), "scs", 256)])
def test_vectorised_apply_is_the_entry_by_entry_apply(matrix, fmt, sigma):
    g, op, plan, sw = plan_of(matrix, fmt, 64, sigma)
    dinv = op.to_dev(pcg_ref.jacobi(g))
    for special in (False, True):
        r = ref.probe_vector(g.nr, 7, special)
        z = plan.apply(r, dinv)[0]
        want = ref.apply_scalar(sw, r, dinv)
        na = np.isnan(z)
        assert np.array_equal(na, np.isnan(want)) and np.array_equal(z.view(np.uint64)[~na], want.view(np.uint64)[~na])
        assert na.any() == special
    g.free()


def dev_matrix(g, op):
    A = pcg_ref.csr(g).tocsr()
    if op.o2n is None:
        return A
    return A[op.n2o][:, op.n2o].tocsr()


@pytest.mark.parametrize("matrix,fmt,sigma", [(("dims", 5, 5, 5), "crs", 1), (("hpcg", 16), "scs", 256), (("irregular", 12), "crs", 1),
                                              (("scaled", 8), "crs", 1)])
def test_apply_is_two_triangular_solves_and_symmetric(matrix, fmt, sigma, tmp):
    """z = (D + U)^-1 D (D + L)^-1 r on the colour-permuted matrix; the contract and scipy's solves round differently: a few
    ulps of ||z|| (the stencils' M is well conditioned; bound 64 eps ||z||)"""
    pytest.importorskip("scipy")
    import scipy.sparse as sp
    import scipy.sparse.linalg as sl
    g, op, plan, sw = plan_of(matrix, fmt, 64, sigma, tmp)
    A = dev_matrix(g, op)
    perm = np.argsort(sw.colour, kind="stable")  # colour order, rows ascending within a colour
    B = A[perm][:, perm].tocsr()
    d = B.diagonal()
    assert np.array_equal(d, op.to_dev(pcg_ref.diagonal(g))[perm])
    DL, DU = sp.tril(B, 0).tocsr(), sp.triu(B, 0).tocsr()
    dinv = op.to_dev(pcg_ref.jacobi(g))
    rng = np.random.RandomState(3)
    u, v = rng.standard_normal(g.nr), rng.standard_normal(g.nr)
    zu, zv = plan.apply(u, dinv)[0], plan.apply(v, dinv)[0]
    want = sl.spsolve_triangular(DU, d * sl.spsolve_triangular(DL, u[perm], lower=True), lower=False)
    err = np.linalg.norm(zu[perm] - want) / np.linalg.norm(want)
    print("apply against scipy's triangular solves", matrix, err)
    assert err <= 64 * np.finfo(float).eps
    a, b = float(u @ zv), float(v @ zu)
    print("symmetry", matrix, a, b)
    assert abs(a - b) <= 64 * np.finfo(float).eps * np.linalg.norm(u) * np.linalg.norm(zv)
    g.free()


def scipy_gap(c, tmp):
    """as test_pcg_host.scipy_gap, with M the restatement's own apply as a LinearOperator"""
    import scipy.sparse.linalg as sl
    plan, _, op, b, dinv, eps = ref.build_case(ref.SGS, c, tmp)
    g = plan.lev[0].g
    assert op.o2n is None
    ours = ref.solve(op, plan, b, dinv, c["itermax"], eps, keep_x=True)
    xs = ours["xs"]
    A = pcg_ref.csr(g)
    M = sl.LinearOperator(A.shape, matvec=lambda r: plan.apply(np.asarray(r, dtype=np.float64).ravel(), dinv)[0], dtype=np.float64)
    theirs = []
    sl.cg(A, b, x0=np.zeros(len(b)), rtol=0.0, atol=0.0, maxiter=len(xs), M=M, callback=lambda xk: theirs.append(xk.copy()))
    assert len(theirs) == len(xs) >= 5
    gap = max(float(np.linalg.norm(a - t) / np.linalg.norm(a)) for a, t in zip(xs, theirs))
    true_res = float(np.linalg.norm(b - A @ ours["x"]))
    g.free()
    return gap, true_res, eps, ours["k"]


@pytest.mark.parametrize("name", ["irregular12", "hpcg16"])
def test_restatement_is_pcg_against_scipy(name, tmp, golden):
    """test_pcg_host.py's bound: 10 x the recorded value, and the recorded value is rounding (< 1e-14)"""
    pytest.importorskip("scipy")
    c = sgs_cases.SCIPY_CASES[name]
    gap, true_res, eps, k = scipy_gap(c, tmp)
    rec = golden["scipy_gap"][name]
    print("scipy_gap", name, gap, "recorded", rec, "k", k, "true residual / eps", true_res / eps)
    assert 0.0 < rec < 1e-14
    assert gap <= 10.0 * rec
    assert k < c["itermax"]
    assert true_res <= 10.0 * eps


def test_diagonal_matrix_is_jacobi_pcg_bit_for_bit(tmp):
    g, op, plan, sw = plan_of(("file", sgs_cases.hand_made("diagonal", tmp)))
    assert sw.nC == 1
    b = np.arange(1.0, g.nr + 1.0) * (-1.0) ** np.arange(g.nr)
    dinv = pcg_ref.jacobi(g)
    got, want = ref.solve(op, plan, b, dinv, 10, 0.0), pcg_ref.solve(op, b, dinv, 10, 0.0)
    assert got["k"] == want["k"]
    for key in ("rr", "rz", "pAp", "x"):
        a, w = got[key], want[key]
        na = np.isnan(a)
        assert np.array_equal(na, np.isnan(w)) and np.array_equal(a.view(np.uint64)[~na], w.view(np.uint64)[~na]), key
    g.free()


@pytest.mark.parametrize("name", list(sgs_cases.COUNT_CASES))
def test_iteration_count_drops_against_jacobi(name, tmp, golden):
    c = sgs_cases.COUNT_CASES[name]
    plan, _, op, b, dinv, eps = ref.build_case(ref.SGS, c, tmp)
    g = plan.lev[0].g
    k_sgs = ref.solve(op, plan, b, dinv, c["itermax"], eps)["k"]
    k_jacobi = pcg_ref.solve(op, b, dinv, c["itermax"], eps)["k"]
    print(name, "k_jacobi", k_jacobi, "k_sgs", k_sgs)
    assert k_sgs < k_jacobi < c["itermax"]
    assert golden["counts"][name] == dict(k_jacobi=k_jacobi, k_sgs=k_sgs, nC=plan.lev[0].smoother.nC)
    g.free()


@pytest.mark.parametrize("name", sgs_cases.SMALL)
def test_the_committed_golden_is_what_the_restatement_gives(name, tmp, golden):
    out = ref.run_case(ref.SGS, sgs_cases.CASES[name], tmp)
    rec = pcg_ref.record(out)
    rec["nC"] = out["nC"]
    assert rec == golden["cases"][name]
    assert set(golden["cases"]) == set(sgs_cases.CASES)
