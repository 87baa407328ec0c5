"""The P-rank restatement of PCG (tests/pcg_mpi_ref.py) checked without a GPU:
  1. on one rank it is pcg_ref.solve, and with the polynomial precond_ref.solve, bit for bit;
  2. with dinv = 1 on 2, 3 and 4 ranks it is the oracle's P-rank CG in the tree order with the pairwise rank sum, bit for bit;
  3. it is PCG of the assembled global system: its iterates against scipy.sparse.linalg.cg with the same preconditioner, under
     the comparison and the bound of tests/test_pcg_host.py and tests/test_poly_host.py;
  4. the polynomial's lmax is the one-rank row bound of the assembled matrix exactly;
  5. the ranks' level-1 values reduced by levels 1-2 and added over ranks (pcg_ref.update_r per rank) are the loop's dots;
  6. tests/golden/pcg_mpi_hist.json (data) equals a fresh run of the restatement bit for bit.
"""
import numpy as np
import pytest

from oracle import pyoracle as po

import pcg_mpi_ref as ref
import pcg_ref
import precond_ref
from conftest import load_json
from test_pcg_host import same


@pytest.fixture(scope="module")
def golden():
    return load_json("pcg_mpi_hist.json")


ONE_RANK = [("crs", 64, 1, 16), ("scs", 64, 256, 16), ("scs", 4, 8, 8)]


@pytest.mark.parametrize("fmt,Cc,sigma,n", ONE_RANK)
def test_one_rank_is_the_one_rank_restatement_bit_for_bit(fmt, Cc, sigma, n):
    R = ref.Ranks.generate(n, 1, fmt, Cc, sigma)
    g, op = R.locs[0], R.ops[0]
    assert g.nc == g.nr and R.plan[0]["externalCount"] == 0
    for dinv in (R.jacobi()[0], ref.caller_dinv(R)[0]):
        got, want = ref.solve(R, [dinv], 40, 0.0), pcg_ref.solve(op, g.rhs(), dinv, 40, 0.0)
        assert got["k"] == want["k"]
        for key in ("rr", "rz", "pAp"):
            assert same(got[key], want[key]), key
        assert same(got["x"][0], want["x"])
    for kw in (dict(steps=1), dict(steps=3), dict(steps=3, lmax=1.75, ratio=8.0)):
        plan = precond_ref.poly(g, op, **kw)
        want = precond_ref.solve(op, plan, g.rhs(), R.jacobi()[0], 40, 0.0)
        got = ref.solve(R, R.jacobi(), 40, 0.0, poly=kw)
        assert got["k"] == want["k"] and got["interval"] == (plan.lev[0].smoother.c["lmin"], plan.lev[0].smoother.c["lmax"])
        for key in ("rr", "rz", "pAp"):
            assert same(got[key], want[key]), (kw, key)
        assert same(got["x"][0], want["x"]), kw
    R.free()


IDENTITY = [("scs", 64, 256, 16, 2, 60), ("scs", 64, 1, 16, 4, 60), ("crs", 64, 1, 16, 2, 60), ("scs", 4, 8, 8, 3, 40),
            ("crs", 64, 1, 8, 3, 40), ("scs", 64, 256, 8, 4, 40)]


@pytest.mark.parametrize("fmt,Cc,sigma,n,P,itermax", IDENTITY)
def test_identity_preconditioner_is_the_oracles_cg_on_p_ranks_bit_for_bit(fmt, Cc, sigma, n, P, itermax):
    R = ref.Ranks.generate(n, P, fmt, Cc, sigma)
    want = po.cg(R.locs, R.plans, itermax=itermax, fmt=fmt, Cc=Cc, sigma=sigma, dot="tree", rank_sum="tree", want_x=True)
    got = ref.solve(R, [np.ones(g.nr) for g in R.locs], itermax, 0.0)
    assert got["k"] == want["k"]
    assert same(got["rr"], want["rr"]) and same(got["pAp"], want["pAp"]) and same(got["rz"], got["rr"])
    for q in range(P):
        assert same(got["x"][q], want["x"][q]), q
    R.free()


def test_identity_on_the_irregular_stand_in_three_ranks():
    R = ref.Ranks.irregular(12, 3, "scs", 64, 256)
    assert all(pl["indegree"] == 2 for pl in R.plan)  # every rank a neighbour of every other
    want = po.cg(R.locs, R.plans, itermax=40, fmt="scs", Cc=64, sigma=256, dot="tree", rank_sum="tree", want_x=True)
    got = ref.solve(R, [np.ones(g.nr) for g in R.locs], 40, 0.0)
    assert got["k"] == want["k"] and same(got["rr"], want["rr"]) and same(got["pAp"], want["pAp"])
    assert all(same(a, b) for a, b in zip(got["x"], want["x"]))
    R.free()


# against scipy's preconditioned CG of the assembled system: name -> (workload, n per rank, P, preconditioner, poly arguments)
SCIPY_CASES = {
    "hpcg16_x2_jacobi": ("hpcg", 16, 2, "jacobi", None), "hpcg16_x3_jacobi": ("hpcg", 16, 3, "jacobi", None),
    "hpcg16_x4_jacobi": ("hpcg", 16, 4, "jacobi", None),
    "hpcg16_x2_caller": ("hpcg", 16, 2, "caller", None), "hpcg16_x3_caller": ("hpcg", 16, 3, "caller", None),
    "hpcg16_x4_caller": ("hpcg", 16, 4, "caller", None),
    "hpcg16_x2_poly": ("hpcg", 16, 2, "poly", dict(steps=3)), "hpcg16_x3_poly": ("hpcg", 16, 3, "poly", dict(steps=3)),
    "hpcg16_x4_poly": ("hpcg", 16, 4, "poly", dict(steps=3)),
    "irregular12_x3_jacobi": ("irregular", 12, 3, "jacobi", None), "irregular12_x3_poly": ("irregular", 12, 3, "poly", dict(steps=3)),
}
ITERMAX = 150


def scipy_gap(case):
    """test_pcg_host.scipy_gap on the assembled system: max_k ||x_k - x_k^scipy|| / ||x_k|| over the iterations both take, the
    true residual at exit, eps and k.  The polynomial's M is the restatement's own apply (test_poly_host.scipy_gap)"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as sl
    workload, n, P, precond, poly = case
    R = (ref.Ranks.irregular if workload == "irregular" else ref.Ranks.generate)(n, P)
    assert all(op.o2n is None for op in R.ops)
    dinv = ref.caller_dinv(R) if precond == "caller" else R.jacobi()
    eps = 1e-10 * R.norm_b()
    ours = ref.solve(R, dinv, ITERMAX, eps, poly=poly, keep_x=True)
    A, b = R.assemble(), np.concatenate(R.rhs())
    if poly is None:
        M = sp.diags(np.concatenate(dinv))
    else:
        plan = ref.Poly(R, R.to_dev(dinv), **poly)
        cuts = np.cumsum([g.nr for g in R.locs])[:-1]
        M = sl.LinearOperator(A.shape, dtype=np.float64,
                              matvec=lambda r: np.concatenate(plan.apply(np.split(np.asarray(r, dtype=np.float64).ravel(), cuts))))
    theirs = []
    sl.cg(A, b, x0=np.zeros(len(b)), rtol=0.0, atol=0.0, maxiter=len(ours["xs"]), M=M, callback=lambda xk: theirs.append(xk.copy()))
    assert len(theirs) == len(ours["xs"]) >= 5
    gap = max(float(np.linalg.norm(a - t) / np.linalg.norm(a)) for a, t in zip(ours["xs"], theirs))
    true_res = float(np.linalg.norm(b - A @ np.concatenate(ours["x"])))
    R.free()
    return gap, true_res, eps, ours["k"]


@pytest.mark.parametrize("name", list(SCIPY_CASES))
def test_restatement_is_pcg_against_scipy(name, golden):
    """test_pcg_host.py's bound: 10 x the value recorded in the golden file, and the recorded value is rounding (< 1e-14)"""
    pytest.importorskip("scipy")
    gap, true_res, eps, k = scipy_gap(SCIPY_CASES[name])
    rec = golden["scipy_gap"][name]
    print("scipy_gap", name, gap, "recorded", rec, "k", k, "true residual / eps", true_res / eps)
    assert 0.0 < rec < 1e-14
    assert gap <= 10.0 * rec
    assert k < ITERMAX  # it converged
    assert true_res <= 10.0 * eps


@pytest.mark.parametrize("workload,n,P,fmt,Cc,sigma", [("hpcg", 8, 2, "crs", 64, 1), ("hpcg", 8, 3, "scs", 4, 8),
                                                        ("hpcg", 8, 4, "scs", 64, 256), ("irregular", 12, 3, "scs", 64, 256)])
def test_lmax_is_the_one_rank_bound_of_the_assembled_matrix(workload, n, P, fmt, Cc, sigma):
    R = (ref.Ranks.irregular if workload == "irregular" else ref.Ranks.generate)(n, P, fmt, Cc, sigma)
    rp, col, val = R.assemble_csr()
    G = po.GMatrix.from_csr(rp.astype(np.uint32), col, val)
    one = precond_ref.rowbound(G, pcg_ref.operator(G), pcg_ref.jacobi(G))
    dinv = R.to_dev(R.jacobi())
    assert R.lmax(dinv) == float(np.max(one))
    # and row for row: the rank's own rows of the one-rank bound, in the rank's device order
    cuts = np.cumsum([g.nr for g in R.locs])[:-1]
    for op, mine, want in zip(R.ops, R.rowbound(dinv), np.split(one, cuts)):
        assert pcg_ref.same_bits(op.to_orig(mine), want)
    G.free(), R.free()


def test_kernel_lines_are_the_loops_lines():
    """the rank's level-1 values reduced by levels 1-2, then the tree over ranks (what the local-reduce kernel and the
    all-reduce make) are the loop's dots; r and z are its waxpby and its product"""
    R = ref.Ranks.generate(8, 3, "scs", 4, 8)
    rng = np.random.RandomState(3)
    r0, Ap = ([rng.standard_normal(g.nr) for g in R.locs] for _ in range(2))
    dinv = R.to_dev(ref.caller_dinv(R))
    r, z, rz, rr = ref.update_r(R, r0, Ap, dinv, -0.375)
    for q in range(R.P):
        assert pcg_ref.same_bits(r[q], po.waxpby(1.0, r0[q], -0.375, Ap[q])) and pcg_ref.same_bits(z[q], r[q] * dinv[q])
    assert rz == R.dot(r, z) and rr == R.dot(r, r)
    R.free()


def test_jacobi_helps_on_several_ranks():
    """the irregular stand-in at 12^3 nodes on 3 ranks: the counts of the one-rank restatements (53 without, 26 with Jacobi)"""
    R = ref.Ranks.irregular(12, 3)
    eps = 1e-10 * R.norm_b()
    k_cg = ref.solve(R, [np.ones(g.nr) for g in R.locs], 150, eps)["k"]
    k_pcg = ref.solve(R, R.jacobi(), 150, eps)["k"]
    k_poly = ref.solve(R, R.jacobi(), 150, eps, poly=dict(steps=3))["k"]
    print("irregular 12^3 nodes x3: k_cg", k_cg, "k_pcg", k_pcg, "k_poly", k_poly)
    assert k_poly < k_pcg < k_cg < 150
    R.free()


@pytest.mark.parametrize("name", list(ref.CASES))
def test_golden_equals_a_fresh_run_of_the_restatement(name, golden):
    assert ref.record(ref.run_case(ref.CASES[name])) == golden["cases"][name]
    assert set(golden["cases"]) == set(ref.CASES)
