"""The CPU restatement of the BiCGStab contract (tests/bicgstab_ref.py) checked without a GPU:
  1. it solves: run to eps = 1e-10 ||b|| it ends with 1 < k < itermax and a TRUE residual ||b - A x||_2 (scipy's CSR product)
     of at most 1.5 eps -- the recursive residual is <= eps at the exit and the gap between the two is of order
     u ||A|| ||x||, about 1e-14 ||b|| on these matrices, so 1.5 is margin;
  2. the Jacobi right preconditioner helps where it should (column-scaled convection-diffusion);
  3. no history value of 59 bodies on convection-diffusion 16^3 is Inf or NaN;
  4. the column-scaled writer writes A S exactly.
"""
import numpy as np
import pytest

import bicgstab_cases as cases
import bicgstab_ref as ref


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("bicgstab")


@pytest.fixture(scope="module")
def runs(tmp):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ref.run_case(cases.HOST_CASES[name], tmp)
        return cache[name]

    return get


@pytest.mark.parametrize("name", list(cases.HOST_CASES))
def test_restatement_solves_to_eps(runs, name):
    c, out = cases.HOST_CASES[name], runs(name)
    k, eps = out["k"], out["eps"]
    true_res = float(np.linalg.norm(out["b"] - out["A"] @ out["x"]))
    print("%s: k = %d, sqrt(rr[-1]) = %.3e, true residual = %.3e = %.3f eps" % (name, k, np.sqrt(out["rr"][-1]), true_res, true_res / eps))
    assert 1 < k < c["itermax"]
    assert len(out["rr"]) == len(out["rho"]) == k and len(out["rv"]) == len(out["ts"]) == len(out["tt"]) == k - 1
    assert np.sqrt(out["rr"][-1]) <= eps < np.sqrt(out["rr"][-2])  # the loop left at the first r.r under eps
    assert true_res <= 1.5 * eps
    assert all(np.isfinite(out[h]).all() for h in ref.HISTORIES)


def test_jacobi_needs_fewer_bodies_on_the_column_scaled_matrix(runs):
    k_none, k_jacobi = runs("scaled_cd16_none")["k"], runs("scaled_cd16_jacobi")["k"]
    print("column-scaled convection-diffusion 16^3, tree order: k = %d without, %d with Jacobi" % (k_none, k_jacobi))
    assert k_jacobi < k_none


def test_histories_stay_finite_without_a_stopping_test(tmp):
    """convection-diffusion 16^3, eps = 0, itermax = 60: 59 bodies well past convergence, every recorded value finite"""
    c = dict(cases.HOST_CASES["cd16"], itermax=60, eps_rel=0.0)
    out = ref.run_case(c, tmp)
    assert out["k"] == 60
    for h in ref.HISTORIES:
        assert np.isfinite(out[h]).all(), (h, np.nonzero(~np.isfinite(out[h]))[0][:5])
    assert len(out["rr"]) == 60 and len(out["tt"]) == 59


def test_first_body_is_the_general_update_on_zero_vectors():
    """p = r + 0.0 * (0 - 0.0 * 0) is r (with -0.0 turned into +0.0, as the kernel's own additions do), ph = p o dinv"""
    r = np.array([1.5, -0.0, 0.0, -2.0, 5e-324])
    dinv = np.array([2.0, 1.0, -1.0, 0.5, 1.0])
    p, ph = ref.update_p(r, np.zeros(5), np.zeros(5), dinv, 0.0, 0.0)
    assert np.array_equal(p, r) and not np.signbit(p[1])
    assert np.array_equal(ph, r * dinv)


def test_scaled_writer_is_a_times_s(tmp):
    a = ref.csr(ref.gmatrix(("cd", 5, 3, 2), tmp)).toarray()
    s = ref.csr(ref.gmatrix(("scaled_cd", 5, 3, 2), tmp)).toarray()
    assert np.array_equal(s, a * cases.scale(np.arange(30))[None, :])
    assert not np.array_equal(a, a.T)  # not symmetric
    assert np.array_equal(ref.jacobi(ref.gmatrix(("scaled_cd", 5, 3, 2), tmp)), 1.0 / (6.0 * cases.scale(np.arange(30))))
