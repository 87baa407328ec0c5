"""The CPU restatement of right-preconditioned GMRES(m) (tests/gmres_precond_ref.py) checked without a GPU:
  1. it is what tests/golden/gmres_precond_hist.json records, bit for bit;
  2. it is GMRES on A M^-1: scipy.sparse.linalg.gmres on the LinearOperator of A M^-1 (no M= argument, same restart) gives the same
     estimate history to within 10 x the recorded gap -- the margin tests/test_gmres_host.py takes, for its reason: scipy's
     orthogonalisation is another one, and the gap moves with the BLAS underneath -- and every recorded gap is below 2e-15 ||b||;
  3. every cycle close's estimate is its explicit residual norm to within 10 x the recorded gap, every recorded gap below
     5e-15 ||b||;
  4. it solves: every converging case ends with 1 < k < itermax and a TRUE residual ||b - A xs||_2 (scipy's CSR product) of at
     most 1.5 eps, after the recorded ratios are shown to be at most 1.0;
  5. the iteration counts of DESIGN 4.20's table are reproduced (gmres_precond_cases.TABLE holds the numbers themselves);
  6. with the identity for M^-1 the wrapper is gmres_ref.solve, bit for bit;
  7. itermax 0 and 1 take no step and return xs = 0;
  8. the launch formula on the restatement's own counts.
"""
import json
import os

import numpy as np
import pytest

import gmres_precond_cases as cases
import gmres_precond_ref as ref
import gmres_ref
import precond_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gmres_precond_hist.json")
same_bits = precond_ref.pcg_ref.same_bits


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("gmres_precond")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_case_list_is_the_one_asked_for():
    assert len(cases.CASES) == 24 and len(cases.HOST_CASES) == 23
    assert all(c["itermax"] == 150 and c["eps_rel"] == 1e-10 for c in cases.CASES.values())
    assert sorted({c["m"] for c in cases.CASES.values()}) == [1, 10, 30]
    assert set(cases.HOST_CASES) - set(cases.CONVERGING) == {"cd16_sell_64_256_signed_m30"}
    d = cases.signed_scale(np.arange(4096))
    assert np.isfinite(d).all() and (d != 0).all() and (d < 0).any() and (d > 0).any()


def test_recorded_gaps_are_rounding(golden):
    for name, rec in golden["cases"].items():
        assert rec["scipy_gap"] < 2e-15 and rec["close_gap"] < 5e-15, (name, rec["scipy_gap"], rec["close_gap"])
        if name in cases.CONVERGING:
            assert rec["true_residual_over_eps"] <= 1.0, (name, rec["true_residual_over_eps"])


@pytest.mark.parametrize("name", list(cases.HOST_CASES))
def test_restatement_is_the_golden_is_scipys_gmres_and_solves(name, tmp, golden):
    c, rec = cases.HOST_CASES[name], golden["cases"][name]
    out = ref.run_case(c, tmp)
    k, eps = out["k"], out["eps"]
    ratio, cg, sg = ref.true_residual_ratio(out), ref.close_gap(out), ref.scipy_gap(c, out, tmp)
    print("%s: k = %d, true residual = %.3f eps, close gap = %.2e, scipy gap = %.2e" % (name, k, ratio, cg, sg))
    assert ref.record(out) == {key: rec[key] for key in ("k", "res", "rr", "x_sha256", "eps", "launches")}
    assert sg <= 10 * max(rec["scipy_gap"], 1e-17)
    assert cg <= 10 * max(rec["close_gap"], 1e-17)
    assert len(out["res"]) == k and np.isfinite(out["res"]).all() and np.isfinite(out["rr"]).all()
    assert len(out["rr"]) == len(out["closes"]) + 1 == 1 + -(-(k - 1) // c["m"])  # the prologue's and one per close
    if name in cases.CONVERGING:
        assert 1 < k < c["itermax"]
        assert out["res"][-1] <= eps < out["res"][-2]
        assert ratio <= 1.5
    else:
        assert k == c["itermax"]


def _key(matrix, m, column):
    return "%s m%d %s" % ("_".join(str(v) for v in matrix), m, column)


@pytest.mark.parametrize("matrix,m", list(cases.TABLE), ids=lambda v: "_".join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_iteration_counts_of_the_table(matrix, m, tmp, golden):
    assert tuple(cases.TABLE[(matrix, m)]) == cases.COLUMNS
    for column, want in cases.TABLE[(matrix, m)].items():
        out = ref.run_case(cases.table_case(matrix, m, column), tmp)
        ratio = ref.true_residual_ratio(out)
        print(matrix, m, column, "k =", out["k"], "true residual = %.3f eps" % ratio)
        assert out["k"] == want == golden["table"][_key(matrix, m, column)], (matrix, m, column)
        assert ratio <= 1.5


@pytest.mark.parametrize("name", ["cd16_sell_64_256_poly_3_16_m10", "cd_10_11_13_sell_64_256_poly_3_16_m1"])
def test_the_identity_is_the_unpreconditioned_solver(name, tmp):
    c = dict(cases.CASES[name], precond="none")
    plan, op, b, eps = ref.build_plan(c, tmp)
    got = ref.solve(op, plan, b, c["m"], c["itermax"], eps)
    want = gmres_ref.solve(op, op.to_dev(b), c["m"], c["itermax"], eps)
    assert got["k"] == want["k"] and 1 < got["k"]
    for key in ("res", "rr"):
        assert same_bits(got[key], want[key]), key
    assert same_bits(got["u"], want["x"]) and same_bits(got["x"], op.to_orig(want["x"]))
    plan.g.free()


@pytest.mark.parametrize("itermax", [0, 1])
def test_no_step_returns_zero(itermax, tmp):
    c = cases.CASES["cd16_sell_64_256_poly_3_16_m10"]
    plan, op, b, eps = ref.build_plan(c, tmp)
    out = ref.solve(op, plan, b, c["m"], itermax, eps)
    assert out["k"] == 1 and len(out["res"]) == len(out["rr"]) == 1 and out["closes"] == []
    assert same_bits(out["x"], np.zeros(len(b))) and same_bits(out["u"], np.zeros(len(b)))
    plan.free()


def test_launch_formula(tmp):
    """a diagonal and one level of one step ride whole: GMRES's own 7 / 8 / 12; the polynomial at 3 steps adds 4 per apply; a
    four-level mgpoly at one step 18; the sweeps their whole cycle"""
    want = {"scaled_cd16_sell_64_256_jacobi_m30": (0, [8, 7, 12]), "cd16_crs_poly_1_16_m30": (0, [8, 7, 12]),
            "cd16_crs_poly_3_16_m30": (4, [12, 11, 20]), "cd16_sell_64_256_poly_3_16_m1": (4, [21]),
            "hpcg16_sell_64_256_mgpoly_galerkin_m30": (18, [26, 25, 48])}
    for name, (A, per) in want.items():
        c = cases.CASES[name]
        plan = ref.build_plan(c, tmp)[0]
        assert ref.apply_launches(plan) == A, name
        assert [ref.launches_per_step(plan, c["m"], j) for j in ref.positions(c["m"])] == per, name
        plan.free() if plan.kind else plan.g.free()
    plan = ref.build_plan(cases.CASES["cd16_crs_sgs_m30"], tmp)[0]
    nC = plan.lev[0].smoother.nC
    assert nC >= 2 and ref.apply_launches(plan) == 2 * nC - 1
    assert ref.launches_per_step(plan, 30, 29) == 12 + 2 * (2 * nC - 1)
    plan.free()


def test_rider_formulas_keep_every_rounding():
    """(v o dinv) * c1 with both products rounded, not v o (dinv * c1)"""
    v, d, c1 = np.array([1.0 + 2.0 ** -52, 3.0, -0.0, np.inf]), np.array([1.0 / 3.0, 1.0 / 7.0, 5.0, 0.0]), 0.1
    a = ref.first(v, d, c1)
    assert same_bits(a[:3], np.array([(v[i] * d[i]) * c1 for i in range(3)])) and np.isnan(a[3])
    assert same_bits(ref.first(v, d)[:3], v[:3] * d[:3]) and np.signbit(ref.first(v, d)[2])
