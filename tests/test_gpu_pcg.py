"""PCG on the GPU == the CPU restatement of its contract (tests/pcg_ref.py, pinned by tests/test_pcg_host.py) BIT
FOR BIT: k, every r.r, every r.z, every p.Ap, x and the preconditioner itself -- Jacobi and a caller's diagonal, every format,
both kernel modes.  With dinv = 1 the solver == hostapi.CG in the tree order bit for bit.  (NaN compares equal to NaN: the
numpy restatement's 0/0 carries the sign bit x86 gives it.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po

import cg_batch_ref
import pcg_cases
import pcg_ref as ref
from conftest import load_json
from sparsebench_amd import hostapi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("pcg_gpu")


def collect(s, k):
    rr, rz, pAp = s.history()
    return dict(k=k, rr=rr, rz=rz, pAp=pAp, x=s.solution(), dinv=s.dinv())


def solve_gpu(p, dinv, itermax, eps):
    s = hostapi.PCG(p, dinv)
    out = collect(s, s.solve(itermax, eps))
    c = s.counters()
    assert c["stop"] == 1 and c["iters"] + 1 == out["k"] and c["n_rr"] == len(out["rr"]) and c["n_pAp"] == len(out["pAp"])
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
    return hostapi.Problem(*ref.problem_args(c["matrix"], tmp), fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])


def modes(p):
    """the kernel modes the matrix has: 5 (masked row programs) where it has them, and 0 (the reference-layout stream)"""
    return sorted({p.use_packed(5), p.use_packed(0)}, reverse=True)


@pytest.mark.parametrize("name", pcg_cases.SMALL)
def test_gpu_equals_the_restatement(gpu, name, tmp):
    c = pcg_cases.CASES[name]
    g, op, b, dinv, eps = ref.build_case(c, tmp)
    want = ref.solve(op, b, dinv, c["itermax"], eps)
    want["dinv"] = dinv
    p = problem(c, tmp)
    assert np.array_equal(p.rhs()[0], b)
    if c["sigma"] > 1:  # the restatement walks the device's own permutation
        assert np.array_equal(p.array("oldToNewPerm"), op.o2n if op.o2n is not None else np.arange(p.nr))
    seen = modes(p)
    if name.startswith("hpcg"):
        assert seen == [5, 0], seen  # the generated stencil in Sell-64 has row programs: both kernels run
    for mode in seen:
        assert p.use_packed(mode) == mode
        got = solve_gpu(p, None if c["dinv"] == "jacobi" else dinv, c["itermax"], eps)
        same(got, want, (name, mode))
    if c["eps_rel"] > 0.0:
        assert 1 < want["k"] < c["itermax"]  # eps was reached in the middle
    s = hostapi.PCG(p)
    fused_dot = (c["fmt"] == "scs" and c["C"] == 64) or p.use_packed(5) == 5
    assert s.launches_per_body() == (5 if fused_dot else 6)
    p.use_packed(0)
    assert s.launches_per_body() == (5 if (c["fmt"] == "scs" and c["C"] == 64) else 6)
    s.free(), p.free(), g.free()


IDENTITY = [("sell_64_256_32", ("hpcg", 32), "scs", 256, 60, 60), ("crs_16", ("hpcg", 16), "crs", 1, 60, 60),
            ("band_klein_crs", ("file", pcg_cases.BAND_KLEIN), "crs", 1, 30, 3), ("band_klein_scs", ("file", pcg_cases.BAND_KLEIN), "scs", 1, 30, 3)]


@pytest.mark.parametrize("name,matrix,fmt,sigma,itermax,expect_k", IDENTITY)
def test_identity_preconditioner_is_hostapi_cg_bit_for_bit(gpu, name, matrix, fmt, sigma, itermax, expect_k, tmp):
    p = hostapi.Problem(*ref.problem_args(matrix, tmp), fmt=fmt, Cc=64, sigma=sigma)
    g = ref.gmatrix(matrix, tmp)
    want = cg_batch_ref.solve(ref.operator(g, fmt, 64, sigma), g.rhs(), itermax, 0.0)
    assert want["k"] == expect_k
    for mode in modes(p):
        p.use_packed(mode)
        got = solve_gpu(p, np.ones(p.nr), itermax, 0.0)
        same(got, want, (name, mode, "restatement of solveCG"), keys=("rr", "pAp", "x"))
        same(dict(k=got["k"], rr=got["rz"]), dict(k=got["k"], rr=got["rr"]), (name, mode, "r.z == r.r"), keys=("rr",))
        assert np.array_equal(got["dinv"], np.ones(p.nr))
        for fused in (1, 0):
            cg = hostapi.CG(p, fused=fused, dot_order="tree")
            k = cg.solve(itermax, 0.0)
            rr, pAp = cg.history()
            same(got, dict(k=k, rr=rr, pAp=pAp, x=cg.solution()), (name, mode, "hostapi.CG fused=%d" % fused), keys=("rr", "pAp", "x"))
            cg.free()
    p.free(), g.free()


def test_loop_edge_cases(gpu, tmp):
    c = pcg_cases.CASES["scaled16_sell_64_256"]
    g, op, b, dinv, eps = ref.build_case(c, tmp)
    p = problem(c, tmp)
    full = ref.solve(op, b, dinv, 150, eps)
    full["dinv"] = dinv
    assert 1 < full["k"] < 150
    # itermax = 1 (and 0): the prologue only
    for im in (1, 0):
        got = solve_gpu(p, None, im, eps)
        want = ref.solve(op, b, dinv, im, eps)
        want["dinv"] = dinv
        same(got, want, ("itermax", im))
        assert got["k"] == 1 and len(got["rr"]) == len(got["rz"]) == 1 and len(got["pAp"]) == 0 and not got["x"].any()
    # in pieces, bodies enqueued well past the exit and past itermax
    s = hostapi.PCG(p)
    s.start(150, eps)
    for _ in range(30):
        s.run_iters(7)
    same(collect(s, s.finish()), full, "pieces")
    assert s.loop_ms() > 0.0
    # the same handle three times: another itermax and eps, then the first solve once more
    short = ref.solve(op, b, dinv, 9, 0.0)
    short["dinv"] = dinv
    same(collect(s, s.solve(9, 0.0)), short, "second solve")
    same(collect(s, s.solve(150, eps)), full, "third solve")
    # a solve abandoned and freed, then the handle's successor on the same matrix
    s.start(150, eps)
    s.run_iters(5)
    s.free()
    same(solve_gpu(p, None, 150, eps), full, "after an abandoned solve")
    p.free(), g.free()


def test_check_residual_and_exact_solution(gpu):
    p = hostapi.Problem("generate", 16, 16, 16, fmt="scs", Cc=64, sigma=256)
    s = hostapi.PCG(p)
    k = s.solve(150, 1e-9)
    assert 1 < k < 150
    x = s.solution()
    assert s.check_residual() == np.max(np.abs(x - 1.0)) < 1e-8
    s.free(), p.free()


@pytest.mark.parametrize("name", [n for n in pcg_cases.CASES if pcg_cases.CASES[n].get("big")])
def test_big_cases_against_the_committed_golden(gpu, name):
    """HPCG 64^3 with the caller's diagonal and 128^3 with Jacobi, 60 iterations: tests/golden/pcg_hist.json, made by the CPU
    restatement"""
    import hashlib
    c = pcg_cases.CASES[name]
    e = load_json("pcg_hist.json")["cases"][name]
    p = problem(c, None)
    dinv = None if c["dinv"] == "jacobi" else pcg_cases.scale(np.arange(p.nr))
    for mode in modes(p):
        p.use_packed(mode)
        got = solve_gpu(p, dinv, c["itermax"], float.fromhex(e["eps"]))
        assert got["k"] == e["k"], (mode, got["k"])
        for key in ("rr", "rz", "pAp"):
            assert ref.same_bits(got[key], ref.unhex(e[key])), (name, mode, key)
        assert hashlib.sha256(np.ascontiguousarray(got["x"]).tobytes()).hexdigest() == e["x_sha256"], (name, mode)
        want_dinv = np.full(p.nr, 1.0 / 27.0) if dinv is None else dinv
        assert ref.same_bits(got["dinv"], want_dinv)
    p.free()


CHILD = r"""
import os
import sys
sys.path.insert(0, %r)
what = sys.argv[1]
if what == "two_ranks":
    os.environ["SB_PACK"] = "0"  # no pattern mirror for the hand-made matrix below
from sparsebench_amd import capi, hostapi
import numpy as np
L = capi.init(0)
if what == "two_ranks":
    # one rank's share of a matrix split over two: 4 rows whose last two columns are halo columns (nc = nr + 2), native CRS
    rowPtr = np.array([0, 2, 5, 8, 10], dtype=np.uint32)
    col = np.array([0, 1, 0, 1, 2, 1, 2, 3, 3, 4], dtype=np.uint32)
    val = np.array([4.0, -1.0, -1.0, 4.0, -1.0, -1.0, 4.0, -1.0, 4.0, -1.0])
    m = L.sb_crs_upload(4, 6, rowPtr.ctypes.data_as(hostapi.vp), col.ctypes.data_as(hostapi.vp), val.ctypes.data_as(hostapi.vp))
    b = np.ones(4)
    L.sb_pcg_create(m, None, b.ctypes.data_as(hostapi.vp), None, None)
elif what == "sp":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1, precision="single")
    b = np.ones(p.nr)
    L.sb_pcg_create(p.matrix, None, b.ctypes.data_as(hostapi.vp), None, None)
elif what == "seq":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    L.sb_set_dot_order(1)
    hostapi.PCG(p)
elif what == "seq_start":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    s = hostapi.PCG(p)
    L.sb_set_dot_order(1)
    s.start(10, 0.0)
elif what in ("zero_diagonal_crs", "zero_diagonal_scs"):
    p = hostapi.Problem(sys.argv[2], 1, 1, 1, fmt=what[-3:], Cc=64, sigma=1)
    hostapi.PCG(p)
elif what == "negative_dinv":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    d = np.ones(p.nr)
    d[37] = -0.5
    hostapi.PCG(p, d)
elif what == "nan_dinv":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="crs")
    d = np.ones(p.nr)
    d[5] = np.nan
    hostapi.PCG(p, d)
print("NOT REFUSED")
"""


def zero_diagonal_file(tmp):
    """a 6 x 6 tridiagonal matrix whose rows 2 and 4 store a 0.0 on the diagonal (row 4 stores it explicitly, row 2 not at all)"""
    path = os.path.join(str(tmp), "zero_diagonal.mtx")
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
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write("6 6 %d\n" % len(ent))
        f.write("".join("%d %d %.17g\n" % (r + 1, c + 1, v) for r, c, v in ent))
    return path


@pytest.mark.parametrize("what,msg", [("two_ranks", "PCG runs on one rank (this process is rank 0 of 1, the matrix has 2 halo columns)"), ("sp", "double precision only"), ("seq", "tree dot order only"),
                                      ("seq_start", "tree dot order only"),
                                      ("zero_diagonal_crs", "2 of 6 matrix rows have no finite positive diagonal entry (the first: device row 2)"),
                                      ("zero_diagonal_scs", "2 of 6 matrix rows have no finite positive diagonal entry (the first: device row 2)"),
                                      ("negative_dinv", "dinv[37] = -0.5"), ("nan_dinv", "dinv[5] = nan")])
def test_refusals_end_the_process_with_their_message(gpu, what, msg, tmp):
    """host-side checks and the diagonal count: fatal with file:line, exit status 1, no GPU fault"""
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT, what, zero_diagonal_file(tmp)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=300)
    err = out.stderr.decode()
    assert out.returncode == 1, (out.returncode, err[-1000:])
    assert msg in err and "sbhip:" in err and "NOT REFUSED" not in out.stdout.decode(), err[-1000:]
    assert "illegal memory access" not in err and "HIP error" not in err
