"""PCG with the full-weighting V-cycle on the GPU == the CPU restatement of its contract (tests/precond_ref.py,
pinned by tests/test_mg_fw_host.py) and tests/golden/mg_fw_hist.json BIT FOR BIT: k, every r.r, every r.z, every p.Ap, x and dinv,
in both kernel modes of the fine matrix's SpMV.  Without coarse levels the solver is hostapi.PCG(precond="sgs") bit for bit; a
second solve on one handle repeats the first; every refusal of sb_pcg_create_mg_p ends the process with its message.  (NaN
compares equal to NaN.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import mg_fw_cases as cases
import pcg_ref
import precond_ref as ref
import sgs_cases
from conftest import load_json
from sparsebench_amd import hostapi
from test_gpu_mg import collect, check_counters, same, same_as_golden, modes, files

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("mg_fw_gpu")


@pytest.fixture(scope="module")
def golden():
    return load_json("mg_fw_hist.json")


def handle(c, tmp):
    """(problem, the coarse problems the caller owns, a constructor of handles) of a case"""
    p = hostapi.Problem(*pcg_ref.problem_args(c["matrix"], tmp), fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])
    if c.get("coarse") is None:
        return p, [], lambda: hostapi.PCG(p, precond="mgfw", levels=c.get("levels"))
    coarse = []
    for (matrix, _, _), (P, omega) in zip(c["coarse"], ref.case_transfers(ref.MGFW, c)):
        q = hostapi.Problem(*pcg_ref.problem_args(matrix, tmp), fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])
        coarse.append((q, P, omega))
    return p, [q for q, _, _ in coarse], lambda: hostapi.PCG(p, precond="mgfw", coarse=coarse)


@pytest.mark.parametrize("name", cases.SMALL)
def test_gpu_equals_the_restatement_and_the_golden(gpu, name, tmp, golden):
    c = cases.CASES[name]
    hier, transfers, op, b, dinv, eps = ref.build_case(ref.MGFW, c, tmp)
    want = ref.solve(op, hier, b, dinv, c["itermax"], eps)
    want["dinv"] = dinv
    e = golden["cases"][name]
    assert eps == float.fromhex(e["eps"]) and e["L"] == hier.L
    p, owned, make = handle(c, tmp)
    assert np.array_equal(p.rhs()[0], b)
    seen = modes(p)
    if name.startswith("hpcg"):
        assert seen == [5, 0], seen
    for mode in seen:
        assert p.use_packed(mode) == mode
        s = make()
        assert s.precond() == "mgfw" and s.levels() == hier.L and [s.level_colours(l) for l in range(hier.L)] == e["nC"]
        assert [s.level_rows(l) for l in range(hier.L)] == e["rows"]
        got = collect(s, s.solve(c["itermax"], eps))
        check_counters(s, got)
        same(got, want, (name, mode))
        same_as_golden(got, e, (name, mode))
        if mode == seen[0]:  # a second solve on the handle repeats the first
            same(collect(s, s.solve(c["itermax"], eps)), got, (name, "again"))
        s.free()
    assert 1 < want["k"] < c["itermax"]  # eps was reached in the middle
    for q in owned:
        q.free()
    p.free(), hier.free()


def test_no_coarse_level_is_sgs_pcg_and_solves_repeat(gpu, tmp):
    c = sgs_cases.CASES["scaled16_sell_64_256"]
    p = hostapi.Problem(*pcg_ref.problem_args(c["matrix"], tmp), fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])
    b = p.rhs()[0]
    eps = 1e-10 * float(np.sqrt(b @ b))
    s = hostapi.PCG(p, precond="sgs")
    want = collect(s, s.solve(150, eps))
    one = hostapi.PCG(p, precond="mgfw", coarse=[])
    assert one.levels() == 1 and one.precond() == "mgfw" and 1 < want["k"] < 150
    same(collect(one, one.solve(150, eps)), want, "no coarse level == SGS")
    # two levels: fewer iterations; in uneven pieces, then another itermax, an apply and a probe in between, then the first again
    coarse = hostapi.Problem("generate", 8, 8, 8, fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])
    two = hostapi.PCG(p, precond="mgfw", coarse=[(coarse, hostapi.mg_trilinear(16, 16, 16), 0.5)])
    first = collect(two, two.solve(150, eps))
    assert first["k"] < want["k"]
    two.start(150, eps)
    for n in (1, 4, 2, 7, 3, 11, 5, 13):
        two.run_iters(n)
    same(collect(two, two.finish()), first, "pieces")
    short = collect(two, two.solve(7, 0.0))
    assert short["k"] == 7
    for key in ("rr", "rz", "pAp"):
        assert pcg_ref.same_bits(short[key][:6], first[key][:6]), key
    z = two.apply(b)
    two.mg_fw_probe(0, b, z, np.ones(512))
    same(collect(two, two.solve(150, eps)), first, "after another solve, an apply and a probe")
    assert np.isfinite(z).all() and two.loop_ms() > 0.0
    same(collect(s, s.solve(150, eps)), want, "SGS after MG")
    two.free(), one.free(), s.free(), coarse.free(), p.free()


def test_check_residual_and_exact_solution(gpu):
    p = hostapi.Problem("generate", 16, 16, 16, fmt="scs", Cc=64, sigma=256)
    s = hostapi.PCG(p, precond="mgfw")
    assert s.levels() == 4  # auto: HPCG's depth
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
p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
ptr, col, val = hostapi.mg_trilinear(8, 8, 8)
omega = 0.5
if what == "sp":
    q = hostapi.Problem("generate", 4, 4, 4, fmt="scs", Cc=64, sigma=1, precision="single")
    q.precision = "double"  # past hostapi's own refusal: the library's is the one under test
elif what == "not_square":  # 4 rows, 6 columns, uploaded directly: no file or generator makes one on a single rank
    class Q:
        precision, nr = "double", 4
        rp, cl, vl = np.array([0, 1, 2, 3, 5], np.uint32), np.array([0, 1, 2, 3, 5], np.uint32), np.array([2.0, 2.0, 2.0, 2.0, -1.0])
        matrix = L.sb_crs_upload(4, 6, rp.ctypes.data_as(hostapi.vp), cl.ctypes.data_as(hostapi.vp), vl.ctypes.data_as(hostapi.vp))
    q = Q()
    col = np.minimum(col, 3)
elif what == "not_smaller":
    q = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
else:
    q = hostapi.Problem(sys.argv[3] if what == "zero_diagonal" else "generate", 4, 4, 4, fmt="scs", Cc=64, sigma=1)
    col = np.minimum(col, q.nr - 1)
if what == "column":
    col[100] = 64
if what == "pointer":
    ptr[201] = ptr[200] - 1
if what == "weight_nan":
    val[33] = np.nan
if what == "weight_inf":
    val[34] = -np.inf
if what.startswith("omega"):
    omega = dict(omega_zero=0.0, omega_negative=-0.5, omega_nan=float("nan"), omega_inf=float("inf"))[what]
    hostapi._omega = lambda omega, l: omega  # past hostapi's own refusal: the library's is the one under test
if what == "seq":
    L.sb_set_dot_order(1)
if what == "fine_zero_diagonal":
    p = hostapi.Problem(sys.argv[3], 1, 1, 1, fmt="crs")
    q = hostapi.Problem(sys.argv[4], 1, 1, 1, fmt="crs")
    ptr, col, val = np.arange(7, dtype=np.uint64), np.array([0, 0, 1, 1, 2, 2], np.uint32), np.ones(6)
hostapi.PCG(p, precond="mgfw", coarse=[(q, (ptr, col, val), omega)])
print("NOT REFUSED")
"""

REFUSALS = [("sp", "sb_pcg_create_mg_p: MG: double precision only (the matrix of level 1"),
            ("not_square", "sb_pcg_create_mg_p: the matrix of level 1 is not square (4 rows, 6 columns)"),
            ("not_smaller", "level 1 has 512 rows, level 0 has 512: every level must be smaller"),
            ("column", "sb_pcg_create_mg_p: level 0: the prolongation's row"),
            ("column", "has column 64 outside the 64 rows of level 1"),
            ("pointer", "sb_pcg_create_mg_p: level 0: the prolongation's row pointer falls from"),
            ("weight_nan", "sb_pcg_create_mg_p: level 0: the prolongation's row"),
            ("weight_nan", "has a weight that is not finite"),
            ("weight_inf", "has a weight that is not finite"),
            ("omega_zero", "sb_pcg_create_mg_p: omega[0] = 0: the restriction's scale of level 0 must be finite and positive"),
            ("omega_negative", "omega[0] = -0.5: the restriction's scale of level 0 must be finite and positive"),
            ("omega_nan", "the restriction's scale of level 0 must be finite and positive"),
            ("omega_inf", "omega[0] = inf: the restriction's scale of level 0 must be finite and positive"),
            ("zero_diagonal", "2 of 6 matrix rows have no finite positive diagonal entry (the first: device row 2): the MG (level 1) preconditioner"),
            ("fine_zero_diagonal", "2 of 6 matrix rows have no finite positive diagonal entry (the first: device row 2): the MG (level 0) preconditioner"),
            ("seq", "tree dot order only")]


@pytest.mark.parametrize("what,msg", REFUSALS)
def test_refusals_end_the_process_with_their_message(gpu, what, msg, tmp):
    """host-side checks and the diagonal count: fatal with file:line, exit status 1, no GPU fault"""
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT, what] + list(files(tmp)), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    err = out.stderr.decode()
    assert out.returncode == 1, (out.returncode, err[-1000:])
    assert msg in err and "sbhip:" in err and "NOT REFUSED" not in out.stdout.decode(), err[-1000:]
    assert "illegal memory access" not in err and "HIP error" not in err


@pytest.mark.parametrize("name", [n for n in cases.CASES if cases.CASES[n].get("big")])
def test_big_case_against_the_committed_golden(gpu, name, golden):
    """HPCG 32^3 at HPCG's depth: tests/golden/mg_fw_hist.json, made by the CPU restatement"""
    c = cases.CASES[name]
    e = golden["cases"][name]
    p = hostapi.Problem(*pcg_ref.problem_args(c["matrix"]), fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])
    for mode in modes(p):
        p.use_packed(mode)
        s = hostapi.PCG(p, precond="mgfw", levels=c["levels"])
        assert [s.level_colours(l) for l in range(s.levels())] == e["nC"] and [s.level_rows(l) for l in range(s.levels())] == e["rows"]
        got = collect(s, s.solve(c["itermax"], float.fromhex(e["eps"])))
        s.free()
        same_as_golden(got, e, (name, mode))
        assert 1 < got["k"] < c["itermax"]
    p.free()
