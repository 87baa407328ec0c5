"""The CPU restatement of the GMRES contract (tests/gmres_ref.py) checked without a GPU:
  1. it is GMRES: its residual estimates against scipy.sparse.linalg.gmres with the same restart length;
  2. on its own: the estimate agrees with the true residual at every cycle close, is non-increasing inside a cycle, and the
     iteration counter / history lengths follow solveCG's convention;
  3. tests/golden/gmres_hist.json (data) equals a fresh run of the restatement bit for bit.
"""
import numpy as np
import pytest

import gmres_cases
import gmres_ref
from conftest import load_json

SMALL = [n for n, c in gmres_cases.CASES.items() if not c.get("big")]


@pytest.fixture(scope="module")
def golden():
    return load_json("gmres_hist.json")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gmres")
    return {n: gmres_ref.run_case(n, tmp) for n in SMALL}, tmp


@pytest.mark.parametrize("name", gmres_cases.SCIPY_CASES)
def test_restatement_is_gmres_against_scipy(name, runs, golden):
    """max_k |res_ours[k] - res_scipy[k]| / ||b||: the two codes orthogonalise differently, so agreement is to rounding of
    ||b||, not bitwise.  Bound: 10 x the value measured with this restatement and recorded in the golden file (the margin
    covers another BLAS summing in another order; it is four orders of magnitude below the first residual drop)."""
    pytest.importorskip("scipy")
    r, tmp = runs
    gap = gmres_ref.scipy_gap(name, r[name], tmp)
    rec = golden["scipy_gap"][name]
    print("scipy_gap", name, gap, "recorded", rec, "k", r[name]["k"])
    assert 0.0 < rec < 2e-15
    assert gap <= 10.0 * rec
    expect_k = {"cd16_m30": 112, "cd16_m10": 111, "cd_10_11_13_m30": 60, "cd16_m1": 150}[name]
    assert r[name]["k"] == expect_k


@pytest.mark.parametrize("name", SMALL)
def test_estimate_true_residual_monotone_and_counter(name, runs, golden):
    r = runs[0][name]
    c = gmres_cases.CASES[name]
    # the estimate against the explicit residual at every cycle close
    gaps = [abs(t - e) / r["bnorm"] for e, t in r["closes"]]
    rec = golden["close_gap"][name]
    print("close_gap", name, max(gaps) if gaps else 0.0, "recorded", rec)
    assert rec < 5e-15
    assert all(g <= 10.0 * rec for g in gaps)
    # inside a cycle the estimate never grows: |sn| <= 1 in IEEE arithmetic
    res, m = r["res"], c["m"]
    for k in range(1, len(res)):
        if (k - 1) % m != 0:  # (step k is the first of a cycle when (k - 1) % m == 0: it starts from the true residual)
            assert res[k] <= res[k - 1], (k, res[k - 1], res[k])
        else:
            assert res[k] <= (res[0] if k == 1 else np.sqrt(r["rr"][(k - 1) // m])), k
    # solveCG's counter: k starts at 1, one estimate per step, k returned
    assert r["k"] == len(res) and 1 <= r["k"] <= c["itermax"]
    steps = r["k"] - 1
    full = steps // m
    open_cycle = 1 if steps % m else 0
    assert len(r["rr"]) == 1 + full + open_cycle == 1 + len(r["closes"])  # (a solve that ends at a full cycle closes it once)


def test_itermax_1_takes_no_step(tmp_path):
    op, b, m, itermax, eps = gmres_ref.build_case("cd_10_11_13_m30", tmp_path)
    for im in (0, 1):
        r = gmres_ref.solve(op, b, m, im, eps)
        assert r["k"] == 1 and len(r["res"]) == 1 and len(r["rr"]) == 1 and not r["x"].any()
    r = gmres_ref.solve(op, b, m, 2, eps)
    assert r["k"] == 2 and len(r["res"]) == 2 and len(r["rr"]) == 2 and r["x"].any()


@pytest.mark.parametrize("name", list(gmres_cases.CASES))
def test_golden_equals_a_fresh_run_of_the_restatement(name, runs, golden):
    """the file is data; the restatement is what pins it"""
    r = runs[0][name] if name in runs[0] else gmres_ref.run_case(name, runs[1])
    assert gmres_ref.record(r) == golden["cases"][name]
