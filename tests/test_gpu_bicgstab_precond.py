"""BiCGStab under PCG's preconditioner plans on the GPU == the CPU restatement of its contract
(tests/bicgstab_precond_ref.py, pinned by tests/test_bicgstab_precond_host.py and recorded in
tests/golden/bicgstab_precond_hist.json) BIT FOR BIT: k, all five histories and x, for every case of
tests/bicgstab_precond_cases.py, in both kernel modes where the matrix has row programs; the launch formula; borrowed, owned and
shared handles; the borrowed PCG handle untouched; the refusals."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bicgstab_precond_cases as cases
import bicgstab_precond_ref as pref
import bicgstab_ref as ref
from sparsebench_amd import hostapi
from test_gpu_bicgstab import collect, modes, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bicgstab_precond_hist.json")
KEYS = ref.HISTORIES + ("x",)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("bicgstab_precond_gpu")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def problem(c, tmp):
    return hostapi.Problem(*ref.problem_args(c["matrix"], tmp), fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])


def plan_args(c):
    """PCG's keyword arguments of a case (not of the device_product one, whose coarse level the test forms)"""
    if c["precond"] == "sgs":
        return {}
    if c["precond"] == "poly":
        return dict(steps=c["steps"], ratio=c["ratio"])
    return dict(steps=c["steps"], ratio=c["ratio"], levels=c["levels"], galerkin=c["galerkin"])


def pcg_of(p, c, owned):
    """the PCG handle of a case over problem p; owned: the coarse problems made here, for the caller to free"""
    if not c.get("device_product"):
        return hostapi.PCG(p, precond=c["precond"], **plan_args(c)), None
    dims = c["matrix"][1:]
    P = hostapi.mg_trilinear(*dims)
    Ac, _ = hostapi.galerkin_product(p, P)
    q = hostapi.Problem.from_csr(*Ac, fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])
    owned.append(q)
    return hostapi.PCG(p, precond="mgpoly", coarse=[(q, P, 1.0)], steps=c["steps"], ratio=c["ratio"]), [Ac]


def check_golden(got, rec, what):
    want = {key: np.array([float.fromhex(v) for v in rec[key]]) for key in ref.HISTORIES}
    want["k"] = rec["k"]
    same(got, want, what, keys=ref.HISTORIES)
    sha = hashlib.sha256(np.ascontiguousarray(got["x"], dtype=np.float64).tobytes()).hexdigest()
    assert sha == rec["x_sha256"], (what, "x")


def solve_collect(s, c, eps):
    out = collect(s, s.solve(c["itermax"], eps))
    del out["dinv"]
    return out


@pytest.mark.parametrize("name", list(cases.CASES))
def test_gpu_equals_the_golden(gpu, name, tmp, golden):
    c = cases.CASES[name]
    p = problem(c, tmp)
    owned = []
    M, coarse_csr = pcg_of(p, c, owned)
    if c.get("device_product"):  # restated here, from the downloaded product
        want = pref.run_case(c, tmp, coarse_csr=coarse_csr)
        assert 1 < want["k"] < c["itermax"]
        rec = pref.record(want)
    else:
        rec = golden[name]
    eps = float.fromhex(rec["eps"])
    seen = modes(p)
    if c["matrix"][0] == "hpcg":
        assert seen == [5, 0], seen  # the generated stencil in Sell-64 has row programs: both kernels run
    for mode in seen:
        assert p.use_packed(mode) == mode
        s = hostapi.BiCGStab(p, precond=M)
        assert s.precond() == c["precond"] and s.launches_per_body() == rec["launches"], (s.precond(), s.launches_per_body())
        assert np.array_equal(s.dinv(), M.dinv())
        check_golden(solve_collect(s, c, eps), rec, (name, mode))
        s.free()
    M.free()
    for q in owned:
        q.free()
    p.free()


def test_launch_formula_against_the_pcg_handles_own_count(gpu, tmp):
    """8 + 2 C under the polynomial, 10 + 2 C under the sweeps, C from PCG's own launches: 4 (+ 1 without a fused dot) + C
    under the polynomial, 6 (+ 1) + C under the sweeps"""
    c = cases.CASES["cd16_sell_64_256_poly_3_16"]
    p = problem(c, tmp)
    for kw, cheb in ((dict(precond="poly", steps=3), True), (dict(precond="poly", steps=1), True), (dict(precond="sgs"), False)):
        s = hostapi.BiCGStab(p, **kw)
        lp = s.pcg.launches_per_body()
        C = [lp - b for b in ((4, 5) if cheb else (6, 7))]
        assert s.launches_per_body() in [(8 if cheb else 10) + 2 * v for v in C], (kw, s.launches_per_body(), lp)
        s.free()
    s = hostapi.BiCGStab(p, precond="poly", steps=3)
    assert s.launches_per_body() == 18
    s.free()
    s = hostapi.BiCGStab(p, precond="poly", steps=1)
    assert s.launches_per_body() == 10
    s.free()
    p.free()


def test_plan_less_pcg_handle_is_the_jacobi_solver(gpu, tmp):
    c = cases.CASES["scaled_cd16_sell_64_256_sgs"]
    p = problem(c, tmp)
    eps = 1e-10 * np.sqrt(p.nr)
    M = hostapi.PCG(p)  # the diagonal, no plan
    a, b = hostapi.BiCGStab(p, precond=M), hostapi.BiCGStab(p, precond="jacobi")
    assert a.precond() == "jacobi" and a.launches_per_body() == b.launches_per_body() == 10
    M.free()  # its dinv was copied: the handle does not refer to it afterwards
    ga, gb = collect(a, a.solve(150, eps)), collect(b, b.solve(150, eps))
    assert 1 < ga["k"] < 150
    same(ga, gb, "plan-less PCG == jacobi")
    # the caller's diagonal travels the same way
    d = ref.bicgstab_cases.scale(np.arange(p.nr))
    M = hostapi.PCG(p, dinv=d)
    a2, b2 = hostapi.BiCGStab(p, precond=M), hostapi.BiCGStab(p, dinv=d)
    same(collect(a2, a2.solve(150, eps)), collect(b2, b2.solve(150, eps)), "plan-less PCG == the caller's dinv")
    for h in (a, b, a2, b2, M):
        h.free()
    p.free()


@pytest.mark.parametrize("name", ["cd16_sell_64_256_poly_3_16", "cd16_sell_64_256_sgs", "hpcg16_sell_64_256_mgpoly_galerkin"])
def test_borrowed_owned_and_shared_handles_give_the_same_bits_and_leave_pcg_alone(gpu, name, tmp, golden):
    c, rec = cases.CASES[name], golden[name]
    eps = float.fromhex(rec["eps"])
    p = problem(c, tmp)
    M = hostapi.PCG(p, precond=c["precond"], **plan_args(c))
    symmetric = c["matrix"][0] == "hpcg"  # PCG itself solves only there; elsewhere its apply is what must not move
    r = np.linspace(-1.0, 2.0, p.nr)
    before = (M.solve(40, 0.0), M.history(), M.solution()) if symmetric else M.apply(r)
    a, b = hostapi.BiCGStab(p, precond=M), hostapi.BiCGStab(p, precond=M)  # two handles on one PCG handle, solved in turn
    owned = hostapi.BiCGStab(p, precond=c["precond"], **plan_args(c))
    assert owned.pcg is not M and owned.precond() == a.precond() == c["precond"]
    ga = solve_collect(a, c, eps)
    gb = solve_collect(b, c, eps)
    ga2 = solve_collect(a, c, eps)
    go = solve_collect(owned, c, eps)
    check_golden(ga, rec, "borrowed")
    for got, what in ((gb, "second handle"), (ga2, "first handle again"), (go, "owned")):
        same(got, ga, what, keys=KEYS)
    # in pieces, the other handle solving in between
    a.start(c["itermax"], eps)
    a.run_iters(3)
    a.run_iters(rec["k"] + 5)
    same(dict(collect(a, a.finish())), ga, "pieces", keys=KEYS)
    after = (M.solve(40, 0.0), M.history(), M.solution()) if symmetric else M.apply(r)
    if symmetric:
        assert before[0] == after[0] and np.array_equal(before[2], after[2])
        assert all(np.array_equal(x, y) for x, y in zip(before[1], after[1]))
    else:
        assert np.array_equal(before, after)
    for h in (a, b, owned, M):
        h.free()
    assert owned.pcg is None
    p.free()


def test_python_refusals(gpu, tmp):
    c = cases.CASES["cd16_crs_poly_3_16"]
    p, q = problem(c, tmp), hostapi.Problem("generate", 8, 8, 8, fmt="crs")
    M = hostapi.PCG(p, precond="poly")
    with pytest.raises(ValueError, match="takes no dinv"):
        hostapi.BiCGStab(p, precond=M, dinv=np.ones(p.nr))
    with pytest.raises(ValueError, match="takes no dinv"):
        hostapi.BiCGStab(p, precond="sgs", dinv=np.ones(p.nr))
    with pytest.raises(ValueError, match="another problem"):
        hostapi.BiCGStab(q, precond=M)
    with pytest.raises(ValueError, match="a PCG handle brings its own"):
        hostapi.BiCGStab(p, precond=M, steps=2)
    with pytest.raises(TypeError, match="go with precond"):
        hostapi.BiCGStab(p, precond="jacobi", steps=2)
    with pytest.raises(ValueError, match="steps, lmax and ratio go with precond='poly' only"):
        hostapi.BiCGStab(p, precond="sgs", steps=2)
    M.free()
    with pytest.raises(ValueError, match="has been freed"):
        hostapi.BiCGStab(p, precond=M)
    p.free(), q.free()


CHILD = r"""
import sys
sys.path.insert(0, %r)
what = sys.argv[1]
from sparsebench_amd import capi, hostapi
import numpy as np
L = capi.init(0)
vp = hostapi.vp
if what == "sp":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1, precision="single")
    b = np.ones(p.nr)
    L.sb_bicgstab_create_pre(p.matrix, None, b.ctypes.data_as(vp), None, None)
else:
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    q = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    b = np.ones(p.nr)
    M = hostapi.PCG(p, precond="poly")
    if what == "other_matrix":
        L.sb_bicgstab_create_pre(q.matrix, None, b.ctypes.data_as(vp), None, M.ptr)
    elif what == "no_handle":
        L.sb_bicgstab_create_pre(p.matrix, None, b.ctypes.data_as(vp), None, None)
    elif what == "open_at_create":
        M.start(10, 0.0)
        hostapi.BiCGStab(p, precond=M)
    elif what == "open_at_start":
        s = hostapi.BiCGStab(p, precond=M)
        M.start(10, 0.0)
        s.start(10, 0.0)
    elif what == "seq":
        L.sb_set_dot_order(1)
        L.sb_bicgstab_create_pre(p.matrix, None, b.ctypes.data_as(vp), None, M.ptr)
    elif what == "closed_again_is_legal":
        s = hostapi.BiCGStab(p, precond=M)
        M.start(10, 0.0)
        M.run_iters(3)
        M.finish()
        assert s.solve(10, 0.0) == 10
        print("SOLVED")
        sys.exit(0)
print("NOT REFUSED")
"""


def child(what):
    return subprocess.run([sys.executable, "-c", CHILD % ROOT, what], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


@pytest.mark.parametrize("what,msg", [("sp", "BiCGStab: double precision only"),
                                      ("other_matrix", "the PCG handle was made over another matrix"),
                                      ("no_handle", "no PCG handle to take the preconditioner from"),
                                      ("open_at_create", "sb_bicgstab_create_pre between sb_pcg_start and sb_pcg_finish"),
                                      ("open_at_start", "sb_bicgstab_start between sb_pcg_start and sb_pcg_finish"),
                                      ("seq", "tree dot order only")])
def test_refusals_end_the_process_with_their_message(gpu, what, msg):
    """host-side checks: fatal with file:line, exit status 1, no GPU fault"""
    out = child(what)
    err = out.stderr.decode()
    assert out.returncode == 1, (out.returncode, err[-1000:])
    assert msg in err and "sbhip:" in err and "NOT REFUSED" not in out.stdout.decode(), err[-1000:]
    assert "illegal memory access" not in err and "HIP error" not in err


def test_a_finished_pcg_solve_is_no_obstacle(gpu):
    out = child("closed_again_is_legal")
    assert out.returncode == 0 and "SOLVED" in out.stdout.decode(), out.stderr.decode()[-1000:]
