"""SGS-preconditioned CG on the GPU == the CPU restatement of its contract (tests/precond_ref.py, pinned by
tests/test_sgs_host.py) BIT FOR BIT: k, every r.r, every r.z, every p.Ap, x and dinv, every format, both kernel modes of the
SpMV.  With one colour the solver is Jacobi hostapi.PCG bit for bit, and a Jacobi handle made after an SGS handle still
reproduces pcg_ref.  (NaN compares equal to NaN.)"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import pcg_ref
import precond_ref as ref
import sgs_cases
from conftest import load_json
from sparsebench_amd import hostapi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("sgs_gpu")


def collect(s, k):
    rr, rz, pAp = s.history()
    return dict(k=k, rr=rr, rz=rz, pAp=pAp, x=s.solution(), dinv=s.dinv())


def check_counters(s, out):
    c = s.counters()
    assert c["stop"] == 1 and c["iters"] + 1 == out["k"] and c["n_rr"] == len(out["rr"]) == len(out["rz"]) and c["n_pAp"] == len(out["pAp"])
    assert len(out["pAp"]) == out["k"] - 1 and len(out["rr"]) == max(1, out["k"] - 1)  # one p.Ap per body; r.r: prologue, then bodies 2 ..


def solve_gpu(p, itermax, eps, precond="sgs"):
    s = hostapi.PCG(p, precond=precond)
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


def problem(c, tmp):
    return hostapi.Problem(*pcg_ref.problem_args(c["matrix"], tmp), fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])


def modes(p):
    """the kernel modes the matrix has: 5 (masked row programs) where it has them, and 0 (the reference-layout stream)"""
    return sorted({p.use_packed(5), p.use_packed(0)}, reverse=True)


@pytest.mark.parametrize("name", sgs_cases.SMALL)
def test_gpu_equals_the_restatement(gpu, name, tmp):
    c = sgs_cases.CASES[name]
    plan, _, op, b, dinv, eps = ref.build_case(ref.SGS, c, tmp)
    g, nC = plan.lev[0].g, plan.lev[0].smoother.nC
    want = ref.solve(op, plan, b, dinv, c["itermax"], eps)
    want["dinv"] = dinv
    p = problem(c, tmp)
    assert np.array_equal(p.rhs()[0], b)
    if c["sigma"] > 1:
        assert np.array_equal(p.array("oldToNewPerm"), op.o2n if op.o2n is not None else np.arange(p.nr))
    seen = modes(p)
    if name.startswith("hpcg"):
        assert seen == [5, 0], seen
    for mode in seen:
        assert p.use_packed(mode) == mode
        got = solve_gpu(p, c["itermax"], eps)
        same(got, want, (name, mode))
    if c["eps_rel"] > 0.0:
        assert 1 < want["k"] < c["itermax"]  # eps was reached in the middle
    s = hostapi.PCG(p, precond="sgs")
    assert s.colours() == nC
    fused_dot = (c["fmt"] == "scs" and c["C"] == 64) or p.use_packed(5) == 5
    assert s.launches_per_body() == 2 * nC + 5 + (0 if fused_dot else 1)
    p.use_packed(0)
    assert s.launches_per_body() == 2 * nC + 5 + (0 if (c["fmt"] == "scs" and c["C"] == 64) else 1)
    s.free(), p.free(), g.free()


def test_pieces_second_solve_and_a_jacobi_handle_afterwards(gpu, tmp):
    c = sgs_cases.CASES["scaled16_sell_64_256"]
    plan, _, op, b, dinv, eps = ref.build_case(ref.SGS, c, tmp)
    g = plan.lev[0].g
    p = problem(c, tmp)
    full = ref.solve(op, plan, b, dinv, 150, eps)
    full["dinv"] = dinv
    assert 1 < full["k"] < 150
    # itermax = 1 and 0: the prologue only (one apply, r.r and r.z recorded)
    for im in (1, 0):
        got = solve_gpu(p, im, eps)
        want = ref.solve(op, plan, b, dinv, im, eps)
        want["dinv"] = dinv
        same(got, want, ("itermax", im))
        assert got["k"] == 1 and len(got["rr"]) == len(got["rz"]) == 1 and len(got["pAp"]) == 0 and not got["x"].any()
    s = hostapi.PCG(p, precond="sgs")
    # in uneven pieces, bodies enqueued well past the exit
    s.start(150, eps)
    for n in (1, 4, 2, 7, 3, 11, 5, 13, 1, 9):
        s.run_iters(n)
    out = collect(s, s.finish())
    same(out, full, "pieces")
    check_counters(s, out)
    assert s.loop_ms() > 0.0
    # the same handle again: another itermax and eps, then the first solve once more (equal bits)
    short = ref.solve(op, plan, b, dinv, 9, 0.0)
    short["dinv"] = dinv
    same(collect(s, s.solve(9, 0.0)), short, "second solve")
    again = collect(s, s.solve(150, eps))
    same(again, out, "third solve == first")
    # the apply between two solves leaves the handle as it was
    z = s.apply(b)
    same(dict(k=0, z=z), dict(k=0, z=op.to_orig(plan.apply(op.to_dev(b), op.to_dev(dinv))[0])), "apply", keys=("z",))
    same(collect(s, s.solve(150, eps)), out, "after an apply")
    # a Jacobi handle created after the SGS handle on the same problem still reproduces pcg_ref: nothing existing changed
    want_j = pcg_ref.solve(op, b, dinv, 150, eps)
    want_j["dinv"] = dinv
    same(solve_gpu(p, 150, eps, precond="jacobi"), want_j, "Jacobi after SGS")
    assert full["k"] < want_j["k"]
    s.free(), p.free(), g.free()


@pytest.mark.parametrize("fmt", ["crs", "scs"])
def test_diagonal_matrix_gives_the_bits_of_jacobi(gpu, fmt, tmp):
    p = hostapi.Problem(sgs_cases.hand_made("diagonal", tmp), 1, 1, 1, fmt=fmt, Cc=64, sigma=1)
    s, j = hostapi.PCG(p, precond="sgs"), hostapi.PCG(p)
    assert s.colours() == 1 and s.launches_per_body() == j.launches_per_body() + 2
    a, b = collect(s, s.solve(10, 0.0)), collect(j, j.solve(10, 0.0))
    same(a, b, ("diagonal", fmt))
    s.free(), j.free(), p.free()


def test_check_residual_and_exact_solution(gpu):
    p = hostapi.Problem("generate", 16, 16, 16, fmt="scs", Cc=64, sigma=256)
    s = hostapi.PCG(p, precond="sgs")
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
if what == "sp":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1, precision="single")
    b = np.ones(p.nr)
    L.sb_pcg_create_sgs(p.matrix, None, b.ctypes.data_as(hostapi.vp), None)
elif what == "seq":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    L.sb_set_dot_order(1)
    hostapi.PCG(p, precond="sgs")
elif what in ("zero_diagonal_crs", "zero_diagonal_scs"):
    p = hostapi.Problem(sys.argv[2], 1, 1, 1, fmt=what[-3:], Cc=64, sigma=1)
    hostapi.PCG(p, precond="sgs")
elif what == "apply_inside_a_solve":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    s = hostapi.PCG(p, precond="sgs")
    s.start(10, 0.0)
    s.apply(np.ones(p.nr))
elif what == "colouring_of_a_diagonal_handle":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="crs")
    hostapi.PCG(p).colouring()
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


ZERO_DIAGONAL = "2 of 6 matrix rows have no finite positive diagonal entry (the first: device row 2): the SGS preconditioner"


@pytest.mark.parametrize("what,msg", [("sp", "sb_pcg_create_sgs: PCG: double precision only"), ("seq", "tree dot order only"),
                                      ("zero_diagonal_crs", ZERO_DIAGONAL), ("zero_diagonal_scs", ZERO_DIAGONAL),
                                      ("apply_inside_a_solve", "sb_pcg_apply_precond between sb_pcg_start and sb_pcg_finish"),
                                      ("colouring_of_a_diagonal_handle", "sb_pcg_colouring: the handle has a diagonal preconditioner")])
def test_refusals_end_the_process_with_their_message(gpu, what, msg, tmp):
    """host-side checks and the diagonal count: fatal with file:line, exit status 1, no GPU fault"""
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT, what, zero_diagonal_file(tmp)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=300)
    err = out.stderr.decode()
    assert out.returncode == 1, (out.returncode, err[-1000:])
    assert msg in err and "sbhip:" in err and "NOT REFUSED" not in out.stdout.decode(), err[-1000:]
    assert "illegal memory access" not in err and "HIP error" not in err


@pytest.mark.parametrize("name", [n for n in sgs_cases.CASES if sgs_cases.CASES[n].get("big")])
def test_big_case_against_the_committed_golden(gpu, name):
    """HPCG 64^3, 60 iterations: tests/golden/sgs_hist.json, made by the CPU restatement"""
    c = sgs_cases.CASES[name]
    e = load_json("sgs_hist.json")["cases"][name]
    p = problem(c, None)
    for mode in modes(p):
        p.use_packed(mode)
        s = hostapi.PCG(p, precond="sgs")
        assert s.colours() == e["nC"]
        got = collect(s, s.solve(c["itermax"], float.fromhex(e["eps"])))
        s.free()
        assert got["k"] == e["k"], (mode, got["k"])
        for key in ("rr", "rz", "pAp"):
            assert pcg_ref.same_bits(got[key], pcg_ref.unhex(e[key])), (name, mode, key)
        assert hashlib.sha256(np.ascontiguousarray(got["x"]).tobytes()).hexdigest() == e["x_sha256"], (name, mode)
    p.free()
