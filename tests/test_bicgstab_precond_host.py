"""The CPU restatement of BiCGStab under a preconditioner plan (tests/bicgstab_precond_ref.py) checked without a GPU:
  1. it solves: every host case run to eps = 1e-10 ||b|| ends with 1 < k < itermax and a TRUE residual ||b - A x||_2 (scipy's CSR
     product) of at most 1.5 eps, tests/test_bicgstab_host.py's bound;
  2. it is what tests/golden/bicgstab_precond_hist.json records, bit for bit;
  3. the iteration counts of DESIGN 4.18's table are reproduced (bicgstab_precond_cases.TABLE holds the numbers themselves);
  4. a plan that is a diagonal and nothing else gives bicgstab_ref.solve with that dinv, bit for bit;
  5. the launch formula on the restatement's own counts.
"""
import json
import os

import numpy as np
import pytest

import bicgstab_precond_cases as cases
import bicgstab_precond_ref as ref
import bicgstab_ref
import precond_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bicgstab_precond_hist.json")


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("bicgstab_precond")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_case_list_is_the_one_asked_for():
    assert len(cases.CASES) == 19 and len(cases.HOST_CASES) == 18
    assert all(c["itermax"] == 150 and c["eps_rel"] == 1e-10 for c in cases.CASES.values())


@pytest.mark.parametrize("name", list(cases.HOST_CASES))
def test_restatement_solves_to_eps_and_is_the_golden(name, tmp, golden):
    c = cases.HOST_CASES[name]
    out = ref.run_case(c, tmp)
    k, eps = out["k"], out["eps"]
    true_res = float(np.linalg.norm(out["b"] - out["A"] @ out["x"]))
    print("%s: k = %d, sqrt(rr[-1]) = %.3e, true residual = %.3e = %.3f eps" % (name, k, np.sqrt(out["rr"][-1]), true_res, true_res / eps))
    assert 1 < k < c["itermax"]
    assert len(out["rr"]) == len(out["rho"]) == k and len(out["rv"]) == len(out["ts"]) == len(out["tt"]) == k - 1
    assert np.sqrt(out["rr"][-1]) <= eps < np.sqrt(out["rr"][-2])
    assert true_res <= 1.5 * eps
    assert all(np.isfinite(out[h]).all() for h in ref.HISTORIES)
    assert ref.record(out) == golden["cases"][name]


def _key(matrix, f, column):
    return "%s %s %s" % ("_".join(str(v) for v in matrix), "_".join(str(v) for v in f), column if isinstance(column, str) else "%s_%d" % column)


@pytest.mark.parametrize("matrix,f", list(cases.TABLE), ids=lambda v: "_".join(str(x) for x in v))
def test_iteration_counts_of_the_table(matrix, f, tmp, golden):
    for column, want in cases.TABLE[(matrix, f)].items():
        c = cases.table_case(matrix, f, column)
        out = bicgstab_ref.run_case(c, tmp) if column in ("none", "jacobi") else ref.run_case(c, tmp)
        true_res = float(np.linalg.norm(out["b"] - out["A"] @ out["x"]))
        print(matrix, f, column, "k =", out["k"], "true residual = %.3f eps" % (true_res / out["eps"]))
        assert out["k"] == want == golden["table"][_key(matrix, f, column)], (matrix, f, column)
        assert true_res <= 1.5 * out["eps"]


class Diagonal:
    """a PCG handle without a plan, as the restatement sees it: z = r o dinv"""

    def __init__(self, dinv_dev):
        self.dinv = dinv_dev

    def apply(self, r, dinv=None):
        return r * self.dinv, None


@pytest.mark.parametrize("name", ["scaled_cd16_jacobi", "cd_10_11_13"])
def test_a_plan_less_handle_is_the_diagonal_solver(name, tmp):
    c = dict(bicgstab_ref.bicgstab_cases.HOST_CASES[name], precond="jacobi")
    g, op, b, dinv, eps = bicgstab_ref.build_case(c, tmp)
    want = bicgstab_ref.solve(op, b, dinv, c["itermax"], eps)
    got = ref.solve(op, Diagonal(op.to_dev(dinv)), b, c["itermax"], eps)
    assert got["k"] == want["k"] and 1 < got["k"] < c["itermax"]
    for key in ref.HISTORIES + ("x",):
        assert precond_ref.pcg_ref.same_bits(got[key], want[key]), key
    g.free()


def test_launch_formula(tmp):
    """18 for the polynomial at 3 steps, 10 for one level of one step, 46 for a four-level mgpoly at one step; the sweeps 10 + 2 C"""
    want = {"cd16_crs_poly_3_16": 18, "cd16_crs_poly_1_16": 10, "hpcg16_sell_64_256_mgpoly_regenerated": 46,
            "hpcg16_sell_64_256_mgpoly_galerkin": 46}
    for name, n in want.items():
        hier = ref.build_plan(cases.CASES[name], tmp)[0]
        assert ref.launches_per_body(hier) == n, name
        hier.free()
    hier = ref.build_plan(cases.CASES["cd16_crs_sgs"], tmp)[0]
    nC = hier.lev[0].smoother.nC
    assert nC >= 2 and ref.launches_per_body(hier) == 10 + 2 * (2 * nC - 1)
    hier.free()
