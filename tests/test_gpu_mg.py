"""MG-preconditioned CG on the GPU == the CPU restatement of its contract (tests/precond_ref.py, pinned by
tests/test_mg_host.py) and tests/golden/mg_hist.json BIT FOR BIT: k, every r.r, every r.z, every p.Ap, x and dinv, in both kernel
modes of the fine matrix's SpMV.  With one level the solver is hostapi.PCG(precond="sgs") bit for bit; a second solve on one
handle repeats the first; every refusal of sb_pcg_create_mg ends the process with its message.  (NaN compares equal to NaN.)"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import mg_cases
import pcg_ref
import precond_ref as ref
import sgs_cases
from conftest import load_json
from sparsebench_amd import hostapi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("mg_gpu")


@pytest.fixture(scope="module")
def golden():
    return load_json("mg_hist.json")


def collect(s, k):
    rr, rz, pAp = s.history()
    return dict(k=k, rr=rr, rz=rz, pAp=pAp, x=s.solution(), dinv=s.dinv())


def check_counters(s, out):
    c = s.counters()
    assert c["stop"] == 1 and c["iters"] + 1 == out["k"] and c["n_rr"] == len(out["rr"]) == len(out["rz"]) and c["n_pAp"] == len(out["pAp"])
    assert len(out["pAp"]) == out["k"] - 1 and len(out["rr"]) == max(1, out["k"] - 1)


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


def handle(c, tmp):
    """(problem, the coarse problems the caller owns, a constructor of MG handles) of a case"""
    p = hostapi.Problem(*pcg_ref.problem_args(c["matrix"], tmp), fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])
    if c.get("coarse") is None:
        return p, [], lambda: hostapi.PCG(p, precond="mg", levels=c.get("levels"))
    coarse = []
    for matrix, f2c in c["coarse"]:
        q = hostapi.Problem(*pcg_ref.problem_args(matrix, tmp), fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])
        coarse.append((q, ref.geometric_f2c(f2c[1:]) if isinstance(f2c, tuple) else np.asarray(f2c)))
    return p, [q for q, _ in coarse], lambda: hostapi.PCG(p, precond="mg", coarse=coarse)


def modes(p):
    """the kernel modes the matrix has: 5 (masked row programs) where it has them, and 0 (the reference-layout stream)"""
    return sorted({p.use_packed(5), p.use_packed(0)}, reverse=True)


@pytest.mark.parametrize("name", mg_cases.SMALL)
def test_gpu_equals_the_restatement_and_the_golden(gpu, name, tmp, golden):
    c = mg_cases.CASES[name]
    hier, f2cs, op, b, dinv, eps = ref.build_case(ref.MG, c, tmp)
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
        assert s.levels() == hier.L and [s.level_colours(l) for l in range(hier.L)] == e["nC"]
        assert [s.level_rows(l) for l in range(hier.L)] == e["rows"]
        got = collect(s, s.solve(c["itermax"], eps))
        check_counters(s, got)
        same(got, want, (name, mode))
        same_as_golden(got, e, (name, mode))
        s.free()
    if c["eps_rel"] > 0.0:
        assert 1 < want["k"] < c["itermax"]  # eps was reached in the middle
    for q in owned:
        q.free()
    p.free(), hier.free()


def test_one_level_is_sgs_pcg_and_a_second_solve_repeats_the_first(gpu, tmp):
    c = sgs_cases.CASES["scaled16_sell_64_256"]
    p = hostapi.Problem(*pcg_ref.problem_args(c["matrix"], tmp), fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])
    b = p.rhs()[0]
    eps = 1e-10 * float(np.sqrt(b @ b))
    s = hostapi.PCG(p, precond="sgs")
    want = collect(s, s.solve(150, eps))
    coarse = hostapi.Problem("generate", 8, 8, 8, fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])
    one = hostapi.PCG(p, precond="mg", coarse=[])
    assert one.levels() == 1 and 1 < want["k"] < 150
    same(collect(one, one.solve(150, eps)), want, "one level == SGS")
    # two levels: fewer iterations; in uneven pieces, then the same handle again with another itermax, then the first once more
    two = hostapi.PCG(p, precond="mg", coarse=[(coarse, ref.geometric_f2c((16, 16, 16)))])
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
    same(collect(two, two.solve(150, eps)), first, "after another solve and an apply")
    assert np.isfinite(z).all() and two.loop_ms() > 0.0
    # the SGS handle made before the MG handles still gives its bits: nothing it uses changed
    same(collect(s, s.solve(150, eps)), want, "SGS after MG")
    two.free(), one.free(), s.free(), coarse.free(), p.free()


def test_check_residual_and_exact_solution(gpu):
    p = hostapi.Problem("generate", 16, 16, 16, fmt="scs", Cc=64, sigma=256)
    s = hostapi.PCG(p, precond="mg")
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
f2c = hostapi.mg_f2c(8, 8, 8)
if what == "sp":
    q = hostapi.Problem("generate", 4, 4, 4, fmt="scs", Cc=64, sigma=1, precision="single")
    q.precision = "double"  # past hostapi's own refusal: the library's is the one under test
elif what == "not_square":  # 4 rows, 6 columns, uploaded directly: no file or generator makes one on a single rank
    class Q:
        precision, nr = "double", 4
        rp, col, val = np.array([0, 1, 2, 3, 5], np.uint32), np.array([0, 1, 2, 3, 5], np.uint32), np.array([2.0, 2.0, 2.0, 2.0, -1.0])
        matrix = L.sb_crs_upload(4, 6, rp.ctypes.data_as(hostapi.vp), col.ctypes.data_as(hostapi.vp), val.ctypes.data_as(hostapi.vp))
    q = Q()
    f2c = f2c[:4].copy()
elif what == "not_smaller":
    q = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    f2c = np.arange(512, dtype=np.uint32)
else:
    q = hostapi.Problem(sys.argv[3] if what == "zero_diagonal" else "generate", 4, 4, 4, fmt="scs", Cc=64, sigma=1)
    f2c = f2c[:q.nr].copy()
if what == "out_of_range":
    f2c[5] = 512
if what == "repeated":
    f2c[7] = f2c[3]
if what == "seq":
    L.sb_set_dot_order(1)
if what == "fine_zero_diagonal":
    p = hostapi.Problem(sys.argv[3], 1, 1, 1, fmt="crs")
    q = hostapi.Problem(sys.argv[4], 1, 1, 1, fmt="crs")
    f2c = np.arange(3, dtype=np.uint32)
hostapi.PCG(p, precond="mg", coarse=[(q, f2c)])
print("NOT REFUSED")
"""


def files(tmp):
    """a 6 x 6 tridiagonal matrix whose rows 2 and 4 have no positive diagonal; a sound 3 x 3 one"""
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
    zero = sgs_cases.write_mtx(os.path.join(str(tmp), "zero_diagonal.mtx"), 6, ent)
    three = sgs_cases.write_mtx(os.path.join(str(tmp), "three.mtx"), 3, [(0, 0, 2.0), (1, 1, 2.0), (2, 2, 2.0)])
    return "-", zero, three


REFUSALS = [("sp", "sb_pcg_create_mg: MG: double precision only (the matrix of level 1"),
            ("not_square", "the matrix of level 1 is not square (4 rows, 6 columns)"),
            ("not_smaller", "level 1 has 512 rows, level 0 has 512: every level must be smaller"),
            ("out_of_range", "f2c[0][5] = 512 is outside the 512 rows of level 0"),
            ("repeated", "f2c[0][7] = 6 repeats entry 3"),
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


@pytest.mark.parametrize("name", [n for n in mg_cases.CASES if mg_cases.CASES[n].get("big")])
def test_big_case_against_the_committed_golden(gpu, name, golden):
    """HPCG 64^3 at HPCG's depth, 60 iterations: tests/golden/mg_hist.json, made by the CPU restatement"""
    c = mg_cases.CASES[name]
    e = golden["cases"][name]
    p = hostapi.Problem(*pcg_ref.problem_args(c["matrix"]), fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])
    for mode in modes(p):
        p.use_packed(mode)
        s = hostapi.PCG(p, precond="mg", levels=c["levels"])
        assert [s.level_colours(l) for l in range(s.levels())] == e["nC"] and [s.level_rows(l) for l in range(s.levels())] == e["rows"]
        got = collect(s, s.solve(c["itermax"], float.fromhex(e["eps"])))
        s.free()
        same_as_golden(got, e, (name, mode))
    p.free()
