"""The CPU restatement of the PCG contract (tests/pcg_ref.py) checked without a GPU:
  1. with dinv = 1 it is the restatement of solveCG (tests/cg_batch_ref.py, itself pinned to the oracle) bit for bit;
  2. it is PCG: its iterates against scipy.sparse.linalg.cg with M = diag(dinv);
  3. the preconditioner helps where it should and changes nothing where it cannot;
  4. tests/golden/pcg_hist.json (data) equals a fresh run of the restatement bit for bit.
"""
import numpy as np
import pytest

from oracle import pyoracle as po

import cg_batch_ref
import pcg_cases
import pcg_ref as ref
from conftest import load_json


@pytest.fixture(scope="module")
def golden():
    return load_json("pcg_hist.json")


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("pcg")


def same(a, b):
    """bit for bit, NaN equal to NaN (the 0/0 of a breakdown carries whatever sign the platform gives it)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


IDENTITY = [("crs16", ("hpcg", 16), "crs", 1, 60), ("sell_64_1_16", ("hpcg", 16), "scs", 1, 60),
            ("sell_64_256_32", ("hpcg", 32), "scs", 256, 60), ("crs_10_11_13", ("dims", 10, 11, 13), "crs", 1, 60),
            ("sell_64_256_10_11_13", ("dims", 10, 11, 13), "scs", 256, 60),
            ("band_klein_crs", ("file", pcg_cases.BAND_KLEIN), "crs", 1, 30), ("band_klein_scs", ("file", pcg_cases.BAND_KLEIN), "scs", 1, 30)]


@pytest.mark.parametrize("name,matrix,fmt,sigma,itermax", IDENTITY)
def test_identity_preconditioner_is_cg_bit_for_bit(name, matrix, fmt, sigma, itermax):
    g = ref.gmatrix(matrix)
    op = ref.operator(g, fmt, 64, sigma)
    b = g.rhs()
    want = cg_batch_ref.solve(op, b, itermax, 0.0)
    got = ref.solve(op, b, np.ones(g.nr), itermax, 0.0)
    assert got["k"] == want["k"]
    assert same(got["rr"], want["rr"]) and same(got["pAp"], want["pAp"]) and same(got["x"], want["x"])
    assert same(got["rz"], got["rr"])
    if name.startswith("band_klein"):
        # r.r = 0 after one body, the second body divides 0 by 0: x is NaN everywhere and the loop leaves at k = 3
        assert got["k"] == 3 and got["rr"][-1] == 0.0 and got["pAp"][-1] == 0.0 and np.isnan(got["x"]).all()
    g.free()


@pytest.mark.parametrize("key", ["hpcg32_x1_scs_C64_sigma256", "hpcg32_x1_crs", "hpcg32_x1_scs_C64_sigma1"])
def test_identity_preconditioner_equals_the_committed_tree_golden(key):
    """(tests/golden/cg_hist_tree.json holds no 16^3 entry: its one-rank 32^3 entries, all three formats)"""
    e = load_json("cg_hist_tree.json")[key]
    g = po.GMatrix.generate(e["n"], e["n"], e["n"])
    got = ref.solve(ref.operator(g, e["fmt"], e["C"], e["sigma"]), g.rhs(), np.ones(g.nr), e["itermax"], 0.0)
    assert got["k"] == e["k"]
    assert ref.same_bits(got["rr"], np.array([float(v) for v in e["rr"]])) and ref.same_bits(got["rz"], got["rr"])
    assert ref.same_bits(got["pAp"], np.array([float(v) for v in e["pAp"]]))
    g.free()


def scipy_gap(c, tmp):
    """max_k ||x_k - x_k^scipy|| / ||x_k|| over the iterations both take, and the true residual at exit over eps"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as sl
    g, op, b, dinv, eps = ref.build_case(c, tmp)
    ours = ref.solve(op, b, dinv, c["itermax"], eps, keep_x=True)
    A = ref.csr(g)
    theirs = []
    sl.cg(A, b, x0=np.zeros(len(b)), rtol=0.0, atol=0.0, maxiter=len(ours["xs"]), M=sp.diags(dinv), callback=lambda xk: theirs.append(xk.copy()))
    assert len(theirs) == len(ours["xs"]) >= 5
    gap = max(float(np.linalg.norm(a - t) / np.linalg.norm(a)) for a, t in zip(ours["xs"], theirs))
    true_res = float(np.linalg.norm(b - A @ ours["x"]))
    g.free()
    return gap, true_res, eps, ours["k"]


@pytest.mark.parametrize("name", list(pcg_cases.SCIPY_CASES))
def test_restatement_is_pcg_against_scipy(name, tmp, golden):
    """The two codes sum their dots in different orders, so the iterates agree to rounding, not bitwise.  Bound: 10 x the
    value measured with this restatement and recorded in the golden file; the recorded values themselves must be rounding
    (< 1e-14)."""
    pytest.importorskip("scipy")
    gap, true_res, eps, k = scipy_gap(pcg_cases.SCIPY_CASES[name], tmp)
    rec = golden["scipy_gap"][name]
    print("scipy_gap", name, gap, "recorded", rec, "k", k, "true residual / eps", true_res / eps)
    assert 0.0 < rec < 1e-14
    assert gap <= 10.0 * rec
    assert k < pcg_cases.SCIPY_CASES[name]["itermax"]  # it converged
    assert true_res <= 10.0 * eps


def test_the_preconditioner_helps_where_it_should(tmp):
    def counts(c, itermax_cg):
        g, op, b, dinv, eps = ref.build_case(c, tmp)
        k_pcg = ref.solve(op, b, dinv, c["itermax"], eps)["k"]
        k_cg = cg_batch_ref.solve(op, b, itermax_cg, eps)["k"]
        g.free()
        return k_pcg, k_cg

    k_pcg, k_cg = counts(pcg_cases.SCIPY_CASES["irregular12"], 150)
    print("irregular 12^3 nodes: k_pcg", k_pcg, "k_cg", k_cg)
    assert k_pcg < k_cg < 150
    k_pcg, k_cg = counts(pcg_cases.SCIPY_CASES["scaled16"], 1000)
    print("scaled HPCG 16^3: k_pcg", k_pcg, "k_cg", k_cg)
    assert 4 * k_pcg <= k_cg < 1000
    k_pcg, k_cg = counts(pcg_cases.SCIPY_CASES["hpcg16"], 150)
    print("HPCG 16^3: k_pcg", k_pcg, "k_cg", k_cg)
    assert k_pcg == k_cg < 150  # a constant diagonal: Jacobi scales z, alpha and beta's operands alike


def test_diagonal_rule(tmp):
    g = ref.gmatrix(("scaled", 8), tmp)
    d = ref.diagonal(g)
    assert np.array_equal(d, 27.0 * pcg_cases.scale(np.arange(g.nr)) ** 2)
    # storage order from +0.0: a stored -0.0 diagonal gives +0.0, duplicates add left to right
    h = po.GMatrix.from_csr([0, 2, 5], [0, 1, 1, 0, 1], [-0.0, 1.0, 0.1, 5.0, 0.2])
    assert ref.same_bits(ref.diagonal(h), np.array([0.0, np.float64(0.0) + 0.1 + 0.2]))
    assert np.signbit(ref.diagonal(h)[0]) == False  # noqa: E712
    g.free(), h.free()


def test_itermax_1_takes_no_step():
    g = po.GMatrix.generate(8, 8, 8)
    op = ref.operator(g)
    for im in (0, 1):
        r = ref.solve(op, g.rhs(), ref.jacobi(g), im, 0.0)
        assert r["k"] == 1 and len(r["rr"]) == len(r["rz"]) == 1 and len(r["pAp"]) == 0 and not r["x"].any()
    r = ref.solve(op, g.rhs(), ref.jacobi(g), 2, 0.0)
    assert r["k"] == 2 and len(r["rr"]) == 1 and len(r["pAp"]) == 1 and r["x"].any()
    g.free()


@pytest.mark.parametrize("name", pcg_cases.SMALL)
def test_golden_equals_a_fresh_run_of_the_restatement(name, tmp, golden):
    """the file is data; the restatement is what pins it (the two big cases are checked on the GPU against the file)"""
    assert ref.record(ref.run_case(pcg_cases.CASES[name], tmp)) == golden["cases"][name]
    assert set(golden["cases"]) == set(pcg_cases.CASES)
