"""The CPU restatement of PCG with the Chebyshev polynomial preconditioner (tests/precond_ref.py) pinned before the
GPU is compared with it: the apply is q(D^-1 A) D^-1 r by the three-term recurrence (against scipy's A @ z) and the residual
polynomial is the scaled Chebyshev polynomial; its matrix is symmetric and positive definite; the symmetric row-sum bound is 53/27
on the stencil, scaled or not, where the naive one is useless; the solve is PCG under that operator (against scipy); the
iteration count drops against Jacobi; steps = 1 with c1 = 1 is Jacobi PCG bit for bit; and tests/golden/poly_hist.json holds
what the restatement gives."""
import numpy as np
import pytest

import pcg_cases
import pcg_ref
import poly_cases
import precond_ref as ref
from conftest import load_json

EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def golden():
    return load_json("poly_hist.json")


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("poly")


def plan_of(matrix, fmt="crs", C=64, sigma=1, tmp=None, **kw):
    """(g, operator, the one-level hierarchy, its Cheb)"""
    g = pcg_ref.gmatrix(matrix, tmp)
    op = pcg_ref.operator(g, fmt, C, sigma)
    plan = ref.poly(g, op, **kw)
    return g, op, plan, plan.lev[0].smoother


def dev_matrix(g, op):
    A = pcg_ref.csr(g).tocsr()
    if op.o2n is None:
        return A
    return A[op.n2o][:, op.n2o].tocsr()


def test_coefficients_follow_the_contract_order():
    c = ref.coeffs(3, 2.0, 16.0)
    lmin = 2.0 / 16.0
    theta, delta = (2.0 + lmin) * 0.5, (2.0 - lmin) * 0.5
    sigma = theta / delta
    rho1 = 1.0 / sigma
    rho2 = 1.0 / (2.0 * sigma - rho1)
    rho3 = 1.0 / (2.0 * sigma - rho2)
    assert c["lmin"] == lmin and c["lmax"] == 2.0 and c["c1"] == 1.0 / theta
    assert c["a"][2:] == [rho2 * rho1, rho3 * rho2] and c["b"][2:] == [(2.0 * rho2) / delta, (2.0 * rho3) / delta]
    assert len(ref.coeff_array(c)) == 5 and len(ref.coeff_array(ref.coeffs(1, 2.0))) == 1
    # the pair the GPU tests use for "steps = 1 is Jacobi": c1 is exactly 1.0
    assert ref.coeffs(1, 1.6, 4.0)["c1"] == 1.0


@pytest.mark.parametrize("matrix,fmt,sigma", [(("dims", 5, 5, 5), "crs", 1), (("hpcg", 16), "scs", 256), (("irregular", 12), "crs", 1),
                                              (("scaled", 8), "crs", 1)])
@pytest.mark.parametrize("steps", [1, 2, 3, 4])
def test_apply_is_the_three_term_recurrence(matrix, fmt, sigma, steps, tmp):
    """z_1 = d_1 = D^-1 r / theta;  d_j = rho_j rho_{j-1} d_{j-1} + (2 rho_j / delta) D^-1 (r - A z_{j-1});  z_j = z_{j-1} + d_j, with
    scipy's A @ z.  The two differ by the rounding of one SpMV (at most L terms, L the longest row) and eight elementwise
    operations per step, each relative to quantities no larger than ||z|| in norm (|D^-1 A| has row sums <= 2 on these
    matrices, a_j < 1, b_j < 2): bound steps * (L + 8) eps ||z||"""
    pytest.importorskip("scipy")
    g, op, plan, ch = plan_of(matrix, fmt, 64, sigma, tmp, steps=steps)
    A = dev_matrix(g, op)
    L = int(np.diff(A.indptr).max())
    c = ch.c
    theta, delta = (c["lmax"] + c["lmin"]) / 2, (c["lmax"] - c["lmin"]) / 2
    rng = np.random.RandomState(3)
    r = rng.standard_normal(g.nr)
    dinv = plan.dinv
    d = dinv * r / theta
    z = d.copy()
    rho = delta / theta
    for _ in range(2, steps + 1):
        rn = 1.0 / (2.0 * theta / delta - rho)
        d = rn * rho * d + 2.0 * rn / delta * (dinv * (r - A @ z))
        z = z + d
        rho = rn
    got = plan.apply(r)[0]
    err = np.linalg.norm(got - z) / np.linalg.norm(z)
    print("apply against the recurrence with scipy's SpMV", matrix, steps, err)
    assert err <= steps * (L + 8) * EPS
    g.free()


@pytest.mark.parametrize("steps", [1, 2, 3, 4])
def test_apply_is_symmetric_positive_definite_and_chebyshev(steps):
    """On the 8^3 stencil, default ratio: M = the dense matrix of the apply.  M is symmetric to rounding (n = 512 columns, each an
    apply of O(steps * 35) roundings at entries <= 1: bound 1e-13 absolute), positive definite, and its residual polynomial is
    the scaled Chebyshev polynomial: I - M A = T_s((theta - D^-1 A) / delta) / T_s(sigma), taken densely by T's own recurrence
    (entries of T_k grow to T_s(sigma) < 10 before the division, n = 512 terms per product: bound 1e-11 absolute)."""
    g, op, plan, ch = plan_of(("hpcg", 8), steps=steps)
    n = g.nr
    M = ref.dense_apply(plan)
    asym = float(np.max(np.abs(M - M.T)))
    lam = np.linalg.eigvalsh((M + M.T) * 0.5)
    print("steps", steps, "asymmetry", asym, "eigenvalues of M in", lam[0], lam[-1])
    assert asym <= 1e-13
    assert lam[0] > 0.0
    A = np.zeros((n, n))
    for i in range(n):
        e = np.zeros(n)
        e[i] = 1.0
        A[:, i] = op.spmv(e)
    c = ch.c
    theta, delta = (c["lmax"] + c["lmin"]) / 2, (c["lmax"] - c["lmin"]) / 2
    X = (theta * np.eye(n) - plan.dinv[:, None] * A) / delta
    sigma = theta / delta
    T0, T1, t0, t1 = np.eye(n), X, 1.0, sigma
    for _ in range(steps - 1):
        T0, T1 = T1, 2.0 * X @ T1 - T0
        t0, t1 = t1, 2.0 * sigma * t1 - t0
    gap = float(np.max(np.abs((np.eye(n) - M @ A) - T1 / t1)))
    print("steps", steps, "residual polynomial against Chebyshev", gap, "T_s(sigma)", t1)
    assert gap <= 1e-11
    g.free()


def test_symmetric_bound_is_two_where_the_naive_bound_is_useless(tmp):
    """The generated stencil stores 27 on the diagonal and at most 26 entries of -1 beside it, so the symmetric row sum of an
    interior row is 1 + 26 / 27 = 53 / 27 = 1.963 (with HPCG's own diagonal of 26 it would be 2.0), reached to within an ulp or two
    of 2.0 by the 27 rounded terms.  S A S with powers of two scales D^-1/2 exactly, so the bound is the same bits; the naive row
    sum of D^-1 A is not"""
    seen = []
    for matrix in (("hpcg", 16), ("scaled", 16)):
        g, op, plan, ch = plan_of(matrix, tmp=tmp)
        assert set(pcg_ref.diagonal(g) / (pcg_cases.scale(np.arange(g.nr)) ** 2 if matrix[0] == "scaled" else 1.0)) == {27.0}
        lmax = float(np.max(ch.g))
        naive = ref.naive_bound(g)
        print(matrix, "bound", repr(lmax), "in ulps of 2.0 from 53/27:", (lmax - 53.0 / 27.0) / np.spacing(2.0), "naive", naive)
        assert abs(lmax - 53.0 / 27.0) <= 2 * np.spacing(2.0)
        assert lmax <= 2.0
        assert ch.c["lmax"] == lmax and ch.c["lmin"] == lmax / 16.0
        if matrix[0] == "scaled":
            assert naive > 10.0 * lmax
        else:
            assert abs(naive - 53.0 / 27.0) <= 2 * np.spacing(2.0)
        seen.append(lmax)
        g.free()
    assert seen[0] == seen[1]


def test_rowbound_is_the_same_in_every_row_order(tmp):
    """the bound's row values do not depend on the format: a row's entries keep their storage order under the permutation"""
    g, op, plan, ch = plan_of(("irregular", 12))
    for fmt, C, sigma in (("scs", 64, 256), ("scs", 4, 8)):
        op2 = pcg_ref.operator(g, fmt, C, sigma)
        ch2 = ref.poly(g, op2).lev[0].smoother
        assert pcg_ref.same_bits(op2.to_orig(ch2.g), op.to_orig(ch.g))
    g.free()


def scipy_gap(c, tmp):
    """as test_pcg_host.scipy_gap, with M the restatement's own apply as a LinearOperator"""
    import scipy.sparse.linalg as sl
    plan, _, op, b, dinv, eps = ref.build_case(ref.POLY, c, tmp)
    g = plan.lev[0].g
    assert op.o2n is None
    ours = ref.solve(op, plan, b, dinv, c["itermax"], eps, keep_x=True)
    xs = ours["xs"]
    A = pcg_ref.csr(g)
    M = sl.LinearOperator(A.shape, matvec=lambda r: plan.apply(np.asarray(r, dtype=np.float64).ravel())[0], dtype=np.float64)
    theirs = []
    sl.cg(A, b, x0=np.zeros(len(b)), rtol=0.0, atol=0.0, maxiter=len(xs), M=M, callback=lambda xk: theirs.append(xk.copy()))
    assert len(theirs) == len(xs) >= 5
    gap = max(float(np.linalg.norm(a - t) / np.linalg.norm(a)) for a, t in zip(xs, theirs))
    true_res = float(np.linalg.norm(b - A @ ours["x"]))
    g.free()
    return gap, true_res, eps, ours["k"]


@pytest.mark.parametrize("name", list(poly_cases.SCIPY_CASES))
def test_restatement_is_pcg_against_scipy(name, tmp, golden):
    """test_pcg_host.py's bound: 10 x the recorded value, and the recorded value is rounding (< 1e-14)"""
    pytest.importorskip("scipy")
    c = poly_cases.SCIPY_CASES[name]
    gap, true_res, eps, k = scipy_gap(c, tmp)
    rec = golden["scipy_gap"][name]
    print("scipy_gap", name, gap, "recorded", rec, "k", k, "true residual / eps", true_res / eps)
    assert 0.0 < rec < 1e-14
    assert gap <= 10.0 * rec
    assert k < c["itermax"]
    assert true_res <= 10.0 * eps


@pytest.mark.parametrize("name", list(poly_cases.COUNT_CASES))
def test_iteration_count_drops_against_jacobi(name, tmp, golden):
    c = poly_cases.COUNT_CASES[name]
    plan, _, op, b, dinv, eps = ref.build_case(ref.POLY, c, tmp)
    g = plan.lev[0].g
    k_poly = ref.solve(op, plan, b, dinv, c["itermax"], eps)["k"]
    k_jacobi = pcg_ref.solve(op, b, dinv, c["itermax"], eps)["k"]
    print(name, "k_jacobi", k_jacobi, "k_poly", k_poly)
    assert k_poly < k_jacobi < c["itermax"]
    assert golden["counts"][name] == dict(k_jacobi=k_jacobi, k_poly=k_poly)
    g.free()


def test_one_step_with_c1_one_is_jacobi_pcg_bit_for_bit(tmp):
    g, op, plan, ch = plan_of(("scaled", 8), "scs", 4, 8, tmp, steps=1, lmax=1.6, ratio=4.0)
    assert ch.c["c1"] == 1.0
    b = g.rhs()
    got, want = ref.solve(op, plan, b, pcg_ref.jacobi(g), 40, 0.0), pcg_ref.solve(op, b, pcg_ref.jacobi(g), 40, 0.0)
    assert got["k"] == want["k"]
    for key in ("rr", "rz", "pAp", "x"):
        assert pcg_ref.same_bits(got[key], want[key]), key
    g.free()


def test_kernel_lines_are_the_apply(tmp):
    """update_r's z and step_l1's (d, z) chained are the plan's apply; their level-1 values reduce to the tree dot"""
    from oracle import pyoracle as po
    g, op, plan, ch = plan_of(("dims", 7, 7, 6), "scs", 64, 256, tmp, steps=3)
    rng = np.random.RandomState(5)
    r0, Ap = rng.standard_normal(g.nr), rng.standard_normal(g.nr)
    r, z, l1rz, l1rr = ref.update_r(r0, Ap, plan.dinv, -0.25, ch.c["c1"])
    assert po.reduce_final(l1rr) == po.ddot_tree(r, r) and po.reduce_final(l1rz) == po.ddot_tree(r, z)
    d = z.copy()
    for j in (2, 3):
        d, z, l1 = ref.step_l1(r, op.spmv(z), plan.dinv, d, z, ch.c["a"][j], ch.c["b"][j])
    want = plan.apply(r)
    assert pcg_ref.same_bits(z, want[0]) and pcg_ref.same_bits(d, want[1])
    assert po.reduce_final(l1) == po.ddot_tree(r, z)
    g.free()


@pytest.mark.parametrize("name", poly_cases.SMALL)
def test_the_committed_golden_is_what_the_restatement_gives(name, tmp, golden):
    out = ref.run_case(ref.POLY, poly_cases.CASES[name], tmp)
    rec = pcg_ref.record(out)
    rec["coeffs"] = [float(v).hex() for v in out["coeffs"]]
    assert rec == golden["cases"][name]
    assert set(golden["cases"]) == set(poly_cases.CASES)
