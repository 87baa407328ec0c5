"""Right-preconditioned GMRES(m) on the GPU == the CPU restatement of its contract (tests/gmres_precond_ref.py,
pinned by tests/test_gmres_precond_host.py and recorded in tests/golden/gmres_precond_hist.json) BIT FOR BIT: k, both histories
and x, for every case of tests/gmres_precond_cases.py, in both kernel modes where the matrix has row programs, the fused loop and
the op list; the launch formula; a diagonal of ones == the unpreconditioned handle; borrowed, owned and shared handles (GMRES and
BiCGStab in turn); the borrowed PCG handle untouched; solves in pieces; exits inside and at the end of a cycle; the refusals."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bicgstab_ref
import gmres_precond_cases as cases
import gmres_precond_ref as ref
from sparsebench_amd import hostapi
from test_gpu_bicgstab import modes
from test_gpu_bicgstab_precond import pcg_of, plan_args
from test_gpu_gmres import same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gmres_precond_hist.json")


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("gmres_precond_gpu")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def problem(c, tmp):
    return hostapi.Problem(*bicgstab_ref.problem_args(c["matrix"], tmp), fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])


def unhex(rec):
    return dict(k=rec["k"], res=np.array([float.fromhex(v) for v in rec["res"]]), rr=np.array([float.fromhex(v) for v in rec["rr"]]))


def collect(s, k):
    res, rr = s.history()
    return dict(k=k, res=res, rr=rr, x=s.solution(), counters=s.counters())


def check_golden(got, rec, what):
    want = unhex(rec)
    want["x"] = got["x"]  # (compared by its SHA-256 below)
    same(got, want, what)
    assert ref.x_sha256(got["x"]) == rec["x_sha256"], (what, "x")
    assert got["counters"]["steps"] == rec["k"] - 1 and got["counters"]["cycles"] == len(rec["rr"]) - 1, (what, got["counters"])


def handle(p, c, fused, owned):
    """(GMRES handle, PCG handle to free or None, coarse CSR of the device_product case)"""
    pre, m = c["precond"], c["m"]
    if pre == "jacobi":
        return hostapi.GMRES(p, restart=m, fused=fused, precond="jacobi"), None, None
    if pre == "signed":
        return hostapi.GMRES(p, restart=m, fused=fused, dinv=cases.signed_scale(np.arange(p.nr))), None, None
    if c.get("aggregation"):
        return hostapi.GMRES(p, restart=m, fused=fused, precond="mgpoly", coarsening="aggregation", steps=c["steps"]), None, None
    M, coarse_csr = pcg_of(p, c, owned)
    return hostapi.GMRES(p, restart=m, fused=fused, precond=M), M, coarse_csr


@pytest.mark.parametrize("name", list(cases.CASES))
def test_gpu_equals_the_golden(gpu, name, tmp, golden):
    c = cases.CASES[name]
    p = problem(c, tmp)
    rec = None if c.get("device_product") else golden[name]
    seen = modes(p)
    if c["matrix"][0] == "hpcg":
        assert seen == [5, 0], seen  # the generated stencil in Sell-64 has row programs: both kernels run
    for mode in seen:
        assert p.use_packed(mode) == mode
        for fused in (True, False):
            owned = []
            s, M, coarse_csr = handle(p, c, fused, owned)
            if rec is None:  # restated here, from the downloaded product
                want = ref.run_case(c, tmp, coarse_csr=coarse_csr)
                assert 1 < want["k"] < c["itermax"]
                rec = ref.record(want)
            want_pre = {"signed": "caller"}.get(c["precond"], c["precond"])
            assert s.precond() == want_pre, (s.precond(), want_pre)
            got_l = [s.launches_per_step(j) for j in ref.positions(c["m"])]
            assert got_l == (rec["launches"] if fused else [0] * len(got_l)), (name, fused, got_l)
            if M is not None:
                assert np.array_equal(s.dinv(), M.dinv())
            check_golden(collect(s, s.solve(c["itermax"], float.fromhex(rec["eps"]))), rec, (name, mode, fused))
            s.free()
            if M is not None:
                M.free()
            for q in owned:
                q.free()
    p.free()


def test_launch_formula_against_the_pcg_handles_own_count(gpu, tmp):
    """A from PCG's own launches per body: 4 (+ 1 without a fused dot) + C under the polynomial, of which one rides; 6 (+ 1) + C
    under the sweeps"""
    c = cases.CASES["cd16_sell_64_256_poly_3_16_m10"]
    p = problem(c, tmp)
    for kw, cheb in ((dict(precond="poly", steps=3), True), (dict(precond="poly", steps=1), True), (dict(precond="sgs"), False)):
        s = hostapi.GMRES(p, restart=10, **kw)
        lp = s.pcg.launches_per_body()
        A = [lp - b - (1 if cheb else 0) for b in ((4, 5) if cheb else (6, 7))]
        assert s.launches_per_step(4) in [7 + a for a in A], (kw, s.launches_per_step(4), lp)
        a = s.launches_per_step(4) - 7
        assert s.launches_per_step(0) == 8 + a and s.launches_per_step(9) == 12 + 2 * a
        s.free()
    for kw, per in ((dict(precond="poly", steps=3), [12, 11, 20]), (dict(precond="poly", steps=1), [8, 7, 12]),
                    (dict(precond="jacobi"), [8, 7, 12]), (dict(), [8, 7, 12])):
        s = hostapi.GMRES(p, restart=10, **kw)
        assert [s.launches_per_step(j) for j in (0, 5, 9)] == per, kw
        s.free()
    s = hostapi.GMRES(p, restart=1, precond="poly", steps=3)
    assert s.launches_per_step(0) == 21
    s.free()
    p.free()


@pytest.mark.parametrize("fused", [True, False])
def test_a_diagonal_of_ones_is_the_unpreconditioned_handle(gpu, fused, tmp):
    c = cases.CASES["cd_10_11_13_sell_64_256_poly_3_16_m30"]
    p = problem(c, tmp)
    eps = 1e-10 * np.sqrt(p.nr)
    a = hostapi.GMRES(p, restart=10, fused=fused)
    b = hostapi.GMRES(p, restart=10, fused=fused, dinv=np.ones(p.nr))
    assert a.precond() == "none" and b.precond() == "caller"
    ga, gb = collect(a, a.solve(150, eps)), collect(b, b.solve(150, eps))
    assert 1 < ga["k"] < 150
    same(gb, ga, "ones")
    a.free(), b.free(), p.free()


def test_plan_less_pcg_handle_is_the_jacobi_solver(gpu, tmp, golden):
    name = "scaled_cd16_sell_64_256_jacobi_m30"
    c, rec = cases.CASES[name], golden[name]
    p = problem(c, tmp)
    M = hostapi.PCG(p)  # the diagonal, no plan
    a = hostapi.GMRES(p, restart=30, precond=M)
    assert a.precond() == "jacobi" and [a.launches_per_step(j) for j in (0, 15, 29)] == [8, 7, 12]
    M.free()  # its dinv was copied: the handle does not refer to it afterwards
    check_golden(collect(a, a.solve(c["itermax"], float.fromhex(rec["eps"]))), rec, "plan-less PCG")
    a.free(), p.free()


@pytest.mark.parametrize("name", ["cd16_sell_64_256_poly_3_16_m10", "cd16_sell_64_256_sgs_m30", "hpcg16_sell_64_256_mgpoly_galerkin_m30"])
def test_borrowed_owned_and_shared_handles_give_the_same_bits_and_leave_pcg_alone(gpu, name, tmp, golden):
    c, rec = cases.CASES[name], golden[name]
    eps, m = float.fromhex(rec["eps"]), c["m"]
    p = problem(c, tmp)
    M = hostapi.PCG(p, precond=c["precond"], **plan_args(c))
    symmetric = c["matrix"][0] == "hpcg"  # PCG itself solves only there; elsewhere its apply is what must not move
    r = np.linspace(-1.0, 2.0, p.nr)
    before = (M.solve(40, 0.0), M.history(), M.solution()) if symmetric else M.apply(r)
    a, b = hostapi.GMRES(p, restart=m, precond=M), hostapi.GMRES(p, restart=m, precond=M, fused=False)
    bi = hostapi.BiCGStab(p, precond=M)  # GMRES and BiCGStab alike share one PCG handle in turn
    owned = hostapi.GMRES(p, restart=m, precond=c["precond"], **plan_args(c))
    assert owned.pcg is not M and owned.precond() == a.precond() == c["precond"]
    ga = collect(a, a.solve(c["itermax"], eps))
    kb = bi.solve(c["itermax"], eps)
    hb, xb = bi.history(), bi.solution()
    gb = collect(b, b.solve(c["itermax"], eps))
    ga2 = collect(a, a.solve(c["itermax"], eps))
    go = collect(owned, owned.solve(c["itermax"], eps))
    check_golden(ga, rec, "borrowed")
    for got, what in ((gb, "second handle"), (ga2, "first handle again"), (go, "owned")):
        same(got, ga, what)
    assert bi.solve(c["itermax"], eps) == kb and np.array_equal(bi.solution(), xb)
    assert all(np.array_equal(bi.history()[key], hb[key]) for key in hb)
    # in pieces, the other handles solving in between
    a.start(c["itermax"], eps)
    a.run_steps(3)
    b.solve(c["itermax"], eps)
    a.run_steps(rec["k"] + 5)
    same(collect(a, a.finish()), ga, "pieces")
    after = (M.solve(40, 0.0), M.history(), M.solution()) if symmetric else M.apply(r)
    if symmetric:
        assert before[0] == after[0] and np.array_equal(before[2], after[2])
        assert all(np.array_equal(x, y) for x, y in zip(before[1], after[1]))
    else:
        assert np.array_equal(before, after)
    for h in (a, b, bi, owned, M):
        h.free()
    assert owned.pcg is None
    p.free()


@pytest.mark.parametrize("fused", [True, False])
def test_exits_inside_and_at_the_end_of_a_cycle_return_the_xs_of_their_last_close(gpu, fused, tmp, golden):
    """eps from the golden history so that the loop test trips at cycle position 4 of the first cycle, then exactly at its last
    position; itermax does the same; itermax 0 and 1 take no step and return 0"""
    name = "cd16_sell_64_256_poly_3_16_m10"
    c = cases.CASES[name]
    res = unhex(golden[name])["res"]
    assert res[5] < res[4] and res[10] < res[9] and res[15] < res[14]
    plan, op, b, _ = ref.build_plan(c, tmp)
    p = problem(c, tmp)
    s = hostapi.GMRES(p, restart=10, fused=fused, precond="poly", steps=c["steps"], ratio=c["ratio"])
    for itermax, eps, k, closes in ((150, 0.5 * (res[4] + res[5]), 6, 1), (150, 0.5 * (res[9] + res[10]), 11, 1),
                                    (150, 0.5 * (res[14] + res[15]), 16, 2), (8, 0.0, 8, 1), (11, 0.0, 11, 1), (21, 0.0, 21, 2),
                                    (0, 0.0, 1, 0), (1, 0.0, 1, 0)):
        want = ref.solve(op, plan, b, 10, itermax, eps)
        assert want["k"] == k and len(want["rr"]) == closes + 1, (itermax, eps, want["k"], len(want["rr"]))
        got = collect(s, s.solve(itermax, eps))
        same(got, want, (fused, itermax, eps))
        assert got["x"].any() == (closes > 0)
    plan.free()
    s.free(), p.free()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ["cd16_sell_64_256_poly_3_16_m10", "cd16_sell_64_256_sgs_m30", "scaled_cd16_sell_64_256_jacobi_m30"])
def test_in_pieces_equals_solve(gpu, name, fused, tmp, golden):
    """run_steps in pieces of 7 (steps past the exit are no-ops); with two handles on one PCG handle taking turns piece by piece"""
    c, rec = cases.CASES[name], golden[name]
    eps = float.fromhex(rec["eps"])
    p = problem(c, tmp)
    kw = dict(precond=c["precond"], **({} if c["precond"] == "jacobi" else plan_args(c)))
    a = hostapi.GMRES(p, restart=c["m"], fused=fused, **kw)
    a.start(c["itermax"], eps)
    for _ in range((c["itermax"] + 6) // 7):
        a.run_steps(7)
    check_golden(collect(a, a.finish()), rec, (name, fused, "pieces"))
    if a.pcg is not None:
        b = hostapi.GMRES(p, restart=7, fused=fused, precond=a.pcg)  # another restart length: its cycle is elsewhere at every turn
        want_b = collect(b, b.solve(c["itermax"], eps))
        a.start(c["itermax"], eps), b.start(c["itermax"], eps)
        for _ in range((c["itermax"] + 4) // 5):
            a.run_steps(5), b.run_steps(5)
        check_golden(collect(a, a.finish()), rec, (name, fused, "turns"))
        same(collect(b, b.finish()), want_b, (name, fused, "the other handle's turns"))
        b.free()
    a.free(), p.free()


@pytest.mark.parametrize("kw", [dict(precond="poly", steps=3, ratio=16.0), dict(precond="sgs")], ids=["poly_3_16", "sgs"])
def test_gmres_and_bicgstab_take_turns_on_one_borrowed_plan(gpu, kw, tmp):
    """The two SOLVERS on one PCG handle's plan, both solves open at once and advanced alternately with the PCG handle's own apply
    between the turns: level 0's d (the polynomial) or the forward sums t (the sweeps) are overwritten at every turn, and each
    solver's histories, k and solution are its own uninterrupted run's bit for bit"""
    p = hostapi.Problem(*bicgstab_ref.problem_args(cases.CD16, tmp), fmt="crs")
    eps = 1e-10 * np.sqrt(p.nr)
    M = hostapi.PCG(p, **kw)
    a, bi = hostapi.GMRES(p, restart=7, precond=M), hostapi.BiCGStab(p, precond=M)
    want_a = collect(a, a.solve(40, eps))
    want_k, want_h, want_x = bi.solve(40, eps), bi.history(), bi.solution()
    assert 1 < want_a["k"] <= 40 and 1 < want_k <= 40 and want_a["x"].any() and want_x.any()
    r = np.linspace(-1.0, 2.0, p.nr)
    a.start(40, eps), bi.start(40, eps)
    for _ in range(20):  # 39 steps in fives, 39 bodies in twos: turns past a solver's exit are no-ops
        a.run_steps(5)
        M.apply(r)
        bi.run_iters(2)
        M.apply(r)
    same(collect(a, a.finish()), want_a, (kw, "GMRES in turns"))
    assert bi.finish() == want_k and np.array_equal(bi.solution(), want_x), (kw, "BiCGStab in turns")
    got_h = bi.history()
    assert all(np.array_equal(got_h[key], want_h[key]) for key in want_h), (kw, "BiCGStab's histories")
    for h in (a, bi, M, p):
        h.free()


def test_python_refusals(gpu, tmp):
    c = cases.CASES["cd16_crs_poly_3_16_m30"]
    p, q = problem(c, tmp), hostapi.Problem("generate", 8, 8, 8, fmt="crs")
    M = hostapi.PCG(p, precond="poly")
    with pytest.raises(ValueError, match="takes no dinv"):
        hostapi.GMRES(p, precond=M, dinv=np.ones(p.nr))
    with pytest.raises(ValueError, match="another problem"):
        hostapi.GMRES(q, precond=M)
    with pytest.raises(ValueError, match="a PCG handle brings its own"):
        hostapi.GMRES(p, precond=M, steps=2)
    with pytest.raises(ValueError, match="steps, lmax and ratio go with precond='poly' only"):
        hostapi.GMRES(p, precond="sgs", steps=2)
    M.free()
    with pytest.raises(ValueError, match="has been freed"):
        hostapi.GMRES(p, precond=M)
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
    L.sb_gmres_create_pre(p.matrix, None, b.ctypes.data_as(vp), None, 10, None)
else:
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    q = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    b = np.ones(p.nr)
    M = hostapi.PCG(p, precond="poly")
    if what == "other_matrix":
        L.sb_gmres_create_pre(q.matrix, None, b.ctypes.data_as(vp), None, 10, M.ptr)
    elif what == "no_handle":
        L.sb_gmres_create_pre(p.matrix, None, b.ctypes.data_as(vp), None, 10, None)
    elif what == "restart0":
        L.sb_gmres_create_pre(p.matrix, None, b.ctypes.data_as(vp), None, 0, M.ptr)
    elif what == "open_at_create":
        M.start(10, 0.0)
        hostapi.GMRES(p, precond=M)
    elif what == "open_at_start":
        s = hostapi.GMRES(p, precond=M)
        M.start(10, 0.0)
        s.start(10, 0.0)
    elif what == "seq":
        L.sb_set_dot_order(1)
        L.sb_gmres_create_pre(p.matrix, None, b.ctypes.data_as(vp), None, 10, M.ptr)
    elif what == "zero_dinv":
        d = np.ones(p.nr)
        d[7] = 0.0
        L.sb_gmres_create_dinv(p.matrix, None, b.ctypes.data_as(vp), None, 10, d.ctypes.data_as(vp))
    elif what == "dinv_of_none":
        s = hostapi.GMRES(p)
        s.dinv()
    elif what == "closed_again_is_legal":
        s = hostapi.GMRES(p, restart=4, precond=M)
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


@pytest.mark.parametrize("what,msg", [("sp", "GMRES: double precision only"),
                                      ("other_matrix", "the PCG handle was made over another matrix"),
                                      ("no_handle", "no PCG handle to take the preconditioner from"),
                                      ("restart0", "sb_gmres_create_pre: restart = 0"),
                                      ("open_at_create", "sb_gmres_create_pre between sb_pcg_start and sb_pcg_finish"),
                                      ("open_at_start", "sb_gmres_start between sb_pcg_start and sb_pcg_finish"),
                                      ("seq", "tree dot order only"),
                                      ("zero_dinv", "dinv[7] = 0: the preconditioner's entries must be finite and non-zero"),
                                      ("dinv_of_none", "the handle has no preconditioner")])
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
