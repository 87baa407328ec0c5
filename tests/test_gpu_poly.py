"""PCG with the Chebyshev polynomial preconditioner on the GPU == the CPU restatement of its contract
(tests/precond_ref.py, pinned by tests/test_poly_host.py) and tests/golden/poly_hist.json BIT FOR BIT: k, every r.r, every r.z,
every p.Ap, x and dinv, every format, both kernel modes of the SpMV.  With steps = 1 and c1 = 1.0 the solver is Jacobi
hostapi.PCG bit for bit, and Jacobi and SGS handles made before and after a polynomial handle still give the histories of their
own goldens.  (NaN compares equal to NaN.)"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import pcg_cases
import pcg_ref
import poly_cases
import precond_ref as ref
import sgs_cases
from conftest import load_json
from sparsebench_amd import hostapi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("poly_gpu")


@pytest.fixture(scope="module")
def golden():
    return load_json("poly_hist.json")


def collect(s, k):
    rr, rz, pAp = s.history()
    return dict(k=k, rr=rr, rz=rz, pAp=pAp, x=s.solution(), dinv=s.dinv())


def check_counters(s, out):
    c = s.counters()
    assert c["stop"] == 1 and c["iters"] + 1 == out["k"] and c["n_rr"] == len(out["rr"]) == len(out["rz"]) and c["n_pAp"] == len(out["pAp"])
    assert len(out["pAp"]) == out["k"] - 1 and len(out["rr"]) == max(1, out["k"] - 1)  # one p.Ap per body; r.r: prologue, then bodies 2 ..


def solve_gpu(p, itermax, eps, **kw):
    s = hostapi.PCG(p, **kw)
    out = collect(s, s.solve(itermax, eps))
    check_counters(s, out)
    s.free()
    return out


def same(got, want, what, keys=("rr", "rz", "pAp", "x", "dinv")):
    assert got["k"] == want["k"], (what, "k", got["k"], want["k"])
    for key in keys:
        a, b = np.ascontiguousarray(got[key], dtype=np.float64), np.ascontiguousarray(want[key], dtype=np.float64)
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        na, nb = np.isnan(a), np.isnan(b)
        assert np.array_equal(na, nb), (what, key, "NaN positions differ")
        bad = np.nonzero((a.view(np.uint64) != b.view(np.uint64)) & ~na)[0]
        assert bad.size == 0, (what, key, "first difference at", int(bad[0]), a[bad[0]], b[bad[0]])


def same_as_golden(got, e, what):
    assert got["k"] == e["k"], (what, got["k"], e["k"])
    for key in ("rr", "rz", "pAp"):
        assert pcg_ref.same_bits(got[key], pcg_ref.unhex(e[key])), (what, key)
    assert hashlib.sha256(np.ascontiguousarray(got["x"]).tobytes()).hexdigest() == e["x_sha256"], what


def problem(c, tmp):
    return hostapi.Problem(*pcg_ref.problem_args(c["matrix"], tmp), fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])


def modes(p):
    """the kernel modes the matrix has: 5 (masked row programs) where it has them, and 0 (the reference-layout stream)"""
    return sorted({p.use_packed(5), p.use_packed(0)}, reverse=True)


@pytest.mark.parametrize("name", list(poly_cases.FORMATS))
def test_gpu_equals_the_restatement_and_the_golden(gpu, name, tmp, golden):
    """both solves of the matrix: to eps = 1e-10 ||b||, and 60 fixed iterations with eps = 0"""
    c_eps, c_60 = poly_cases.CASES[name + "_eps"], poly_cases.CASES[name + "_60"]
    plan, _, op, b, dinv, eps = ref.build_case(ref.POLY, c_eps, tmp)
    g = plan.lev[0].g
    p = problem(c_eps, tmp)
    assert np.array_equal(p.rhs()[0], b)
    if c_eps["sigma"] > 1:
        assert np.array_equal(p.array("oldToNewPerm"), op.o2n if op.o2n is not None else np.arange(p.nr))
    seen = modes(p)
    if name.startswith("hpcg"):
        assert seen == [5, 0], seen
    for c, tag, e in ((c_eps, "_eps", eps), (c_60, "_60", 0.0)):
        want = ref.solve(op, plan, b, dinv, c["itermax"], e)
        want["dinv"] = op.to_orig(plan.dinv)
        rec = golden["cases"][name + tag]
        assert float.fromhex(rec["eps"]) == e
        same_as_golden(want, rec, (name, tag, "restatement"))
        for mode in seen:
            assert p.use_packed(mode) == mode
            got = solve_gpu(p, c["itermax"], e, precond="poly")
            same(got, want, (name, tag, mode))
            same_as_golden(got, rec, (name, tag, mode))
        if c["eps_rel"] > 0.0:
            assert 1 < want["k"] < c["itermax"]  # eps was reached in the middle
        else:
            assert want["k"] == c["itermax"]
    fused64 = c_eps["fmt"] == "scs" and c_eps["C"] == 64
    for steps in (1, 2, 3, 4):
        s = hostapi.PCG(p, precond="poly", steps=steps)
        assert p.use_packed(5) in (0, 5)
        assert s.launches_per_body() == 5 + 2 * (steps - 1) + (0 if (fused64 or p.use_packed(5) == 5) else 1)
        p.use_packed(0)
        assert s.launches_per_body() == 5 + 2 * (steps - 1) + (0 if fused64 else 1)
        assert s.precond_bytes() == (steps - 1) * (gpu.sb_matrix_spmv_bytes(p.matrix) + 56.0 * g.nr) + 24.0 * g.nr
        s.free()
    p.free(), g.free()


def test_pieces_second_solve_and_the_other_kinds_around_it(gpu, tmp):
    """start / run_iters / finish in pieces equals solve; the handle solves again; a Jacobi and an SGS handle made BEFORE and AFTER
    the polynomial one in the same process give the histories of their own committed goldens"""
    name = "scaled16_sell_64_256"
    cj, cs = pcg_cases.CASES[name], sgs_cases.CASES[name]
    ej, es = load_json("pcg_hist.json")["cases"][name], load_json("sgs_hist.json")["cases"][name]
    c = poly_cases.CASES[name + "_eps"]
    plan, _, op, b, dinv, eps = ref.build_case(ref.POLY, c, tmp)
    g = plan.lev[0].g
    assert float.fromhex(ej["eps"]) == float.fromhex(es["eps"]) == eps
    p = problem(c, tmp)

    def others(when):
        for mode in modes(p):
            p.use_packed(mode)
            same_as_golden(solve_gpu(p, cj["itermax"], eps, precond="jacobi"), ej, ("Jacobi", when, mode))
            same_as_golden(solve_gpu(p, cs["itermax"], eps, precond="sgs"), es, ("SGS", when, mode))

    others("before")
    p.use_packed(5)
    full = ref.solve(op, plan, b, dinv, 150, eps)
    full["dinv"] = op.to_orig(plan.dinv)
    assert 1 < full["k"] < 150
    # itermax = 1 and 0: the prologue only (one apply, r.r and r.z recorded)
    for im in (1, 0):
        got = solve_gpu(p, im, eps, precond="poly")
        want = ref.solve(op, plan, b, dinv, im, eps)
        want["dinv"] = full["dinv"]
        same(got, want, ("itermax", im))
        assert got["k"] == 1 and len(got["rr"]) == len(got["rz"]) == 1 and len(got["pAp"]) == 0 and not got["x"].any()
    s = hostapi.PCG(p, precond="poly")
    s.start(150, eps)
    for n in (1, 4, 2, 7, 3, 11, 5, 13, 1, 9):  # uneven pieces, bodies enqueued well past the exit
        s.run_iters(n)
    out = collect(s, s.finish())
    same(out, full, "pieces")
    check_counters(s, out)
    assert s.loop_ms() > 0.0
    short = ref.solve(op, plan, b, dinv, 9, 0.0)
    short["dinv"] = full["dinv"]
    same(collect(s, s.solve(9, 0.0)), short, "second solve")
    same(collect(s, s.solve(150, eps)), out, "third solve == first")
    z = s.apply(b)  # the apply between two solves leaves the handle as it was
    same(dict(k=0, z=z), dict(k=0, z=op.to_orig(plan.apply(op.to_dev(b))[0])), "apply", keys=("z",))
    same(collect(s, s.solve(150, eps)), out, "after an apply")
    others("after, the polynomial handle alive")
    s.free()
    others("after")
    assert full["k"] < ej["k"]
    p.free(), g.free()


@pytest.mark.parametrize("fmt,C,sigma", [("crs", 64, 1), ("scs", 64, 256), ("scs", 4, 8)])
def test_one_step_with_c1_one_gives_the_bits_of_jacobi(gpu, fmt, C, sigma, tmp):
    p = hostapi.Problem(*pcg_ref.problem_args(("scaled", 8), tmp), fmt=fmt, Cc=C, sigma=sigma)
    s, j = hostapi.PCG(p, precond="poly", steps=1, lmax=1.6, ratio=4.0), hostapi.PCG(p)
    assert s.coeffs().tolist() == [1.0] and s.interval() == (1.6 / 4.0, 1.6)  # c1 is exactly 1.0: verified, not assumed
    assert s.launches_per_body() == j.launches_per_body()
    for itermax, eps in ((40, 0.0), (150, 1e-8)):
        a, b = collect(s, s.solve(itermax, eps)), collect(j, j.solve(itermax, eps))
        same(a, b, ("c1 = 1", fmt, itermax))
    same(dict(k=0, z=s.apply(p.rhs()[0])), dict(k=0, z=j.apply(p.rhs()[0])), "apply", keys=("z",))
    s.free(), j.free(), p.free()


def test_check_residual_and_exact_solution(gpu):
    p = hostapi.Problem("generate", 16, 16, 16, fmt="scs", Cc=64, sigma=256)
    s = hostapi.PCG(p, precond="poly")
    k = s.solve(150, 1e-9)
    assert 1 < k < 150
    x = s.solution()
    assert s.check_residual() == np.max(np.abs(x - 1.0)) < 1e-8
    s.free(), p.free()


CHILD = r"""
import sys
sys.path.insert(0, %r)
what = sys.argv[1]
from sparsebench_amd import capi, hostapi
import numpy as np
L = capi.init(0)
b = np.ones(512)
if what == "sp":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1, precision="single")
    L.sb_pcg_create_poly(p.matrix, None, b.ctypes.data_as(hostapi.vp), None, 3, 0.0, 0.0)
elif what == "seq":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    L.sb_set_dot_order(1)
    hostapi.PCG(p, precond="poly")
elif what in ("zero_diagonal_crs", "zero_diagonal_scs"):
    p = hostapi.Problem(sys.argv[2], 1, 1, 1, fmt=what[-3:], Cc=64, sigma=1)
    hostapi.PCG(p, precond="poly")
elif what in ("steps_17", "ratio_1", "lmax_inf"):
    p = hostapi.Problem("generate", 8, 8, 8, fmt="crs")
    steps, lmax, ratio = dict(steps_17=(17, 0.0, 0.0), ratio_1=(3, 0.0, 1.0), lmax_inf=(3, float("inf"), 0.0))[what]
    L.sb_pcg_create_poly(p.matrix, None, b.ctypes.data_as(hostapi.vp), None, steps, lmax, ratio)
elif what == "apply_inside_a_solve":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    s = hostapi.PCG(p, precond="poly")
    s.start(10, 0.0)
    s.apply(np.ones(p.nr))
elif what == "interval_of_a_diagonal_handle":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="crs")
    out = np.zeros(2)
    L.sb_pcg_poly_interval(hostapi.PCG(p).ptr, out.ctypes.data_as(hostapi.vp))
print("NOT REFUSED")
"""


def zero_diagonal_file(tmp):
    """a 6 x 6 tridiagonal matrix whose rows 2 and 4 have a 0.0 on the diagonal (row 4 stores it, row 2 stores none)"""
    ent = []
    for i in range(6):
        if i > 0:
            ent.append((i, i - 1, -1.0))
        if i == 4:
            ent.append((i, i, 0.0))
        elif i != 2:
            ent.append((i, i, 4.0))
        if i < 5:
            ent.append((i, i + 1, -1.0))
    return sgs_cases.write_mtx(os.path.join(str(tmp), "zero_diagonal.mtx"), 6, ent)


ZERO_DIAGONAL = ("2 of 6 matrix rows have no finite positive diagonal entry (the first: device row 2): the Chebyshev polynomial "
                 "preconditioner")


@pytest.mark.parametrize("what,msg", [("sp", "sb_pcg_create_poly: PCG: double precision only"), ("seq", "tree dot order only"),
                                      ("zero_diagonal_crs", ZERO_DIAGONAL), ("zero_diagonal_scs", ZERO_DIAGONAL),
                                      ("steps_17", "sb_pcg_create_poly: steps = 17"), ("ratio_1", "sb_pcg_create_poly: ratio = 1"),
                                      ("lmax_inf", "sb_pcg_create_poly: lmax = inf"),
                                      ("apply_inside_a_solve", "sb_pcg_apply_precond between sb_pcg_start and sb_pcg_finish"),
                                      ("interval_of_a_diagonal_handle", "sb_pcg_poly_interval: the handle has another preconditioner")])
def test_refusals_end_the_process_with_their_message(gpu, what, msg, tmp):
    """host-side checks and the diagonal count: fatal with file:line, exit status 1, no GPU fault"""
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT, what, zero_diagonal_file(tmp)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=300)
    err = out.stderr.decode()
    assert out.returncode == 1, (out.returncode, err[-1000:])
    assert msg in err and "sbhip:" in err and "NOT REFUSED" not in out.stdout.decode(), err[-1000:]
    assert "illegal memory access" not in err and "HIP error" not in err


@pytest.mark.parametrize("name", [n for n in poly_cases.CASES if poly_cases.CASES[n].get("big")])
def test_big_case_against_the_committed_golden(gpu, name, golden):
    """HPCG 128^3, Sell-64-256, 20 iterations: tests/golden/poly_hist.json, made by the CPU restatement"""
    c = poly_cases.CASES[name]
    e = golden["cases"][name]
    p = problem(c, None)
    for mode in modes(p):
        p.use_packed(mode)
        s = hostapi.PCG(p, precond="poly")
        assert pcg_ref.same_bits(s.coeffs(), pcg_ref.unhex(e["coeffs"]))
        got = collect(s, s.solve(c["itermax"], float.fromhex(e["eps"])))
        s.free()
        same_as_golden(got, e, (name, mode))
    p.free()
