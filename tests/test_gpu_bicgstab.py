"""BiCGStab on the GPU == the CPU restatement of its contract (tests/bicgstab_ref.py, pinned by
tests/test_bicgstab_host.py) BIT FOR BIT: k, all five histories, x and the preconditioner itself -- none, Jacobi and a caller's
diagonal, every format, both kernel modes.  (NaN compares equal to NaN.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import bicgstab_cases as cases
import bicgstab_ref as ref
from sparsebench_amd import hostapi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ref.HISTORIES + ("x", "dinv")


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("bicgstab_gpu")


def collect(s, k):
    out = dict(s.history(), k=k, x=s.solution(), dinv=s.dinv())
    c = s.counters()
    assert c["stop"] == 1 and c["iters"] + 1 == k, (c, k)
    assert c["n_rr"] == len(out["rr"]) == len(out["rho"]) == k, (c, k)
    assert c["n_rv"] == c["n_ts"] == len(out["rv"]) == len(out["ts"]) == len(out["tt"]) == k - 1, (c, k)
    return out


def handle(p, c, dinv):
    if c["precond"] == "scale":
        return hostapi.BiCGStab(p, dinv=dinv)
    return hostapi.BiCGStab(p, precond=c["precond"])


def same(got, want, what, keys=KEYS):
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


@pytest.mark.parametrize("name", list(cases.CASES))
def test_gpu_equals_the_restatement(gpu, name, tmp):
    c = cases.CASES[name]
    g, op, b, dinv, eps = ref.build_case(c, tmp)
    want = ref.solve(op, b, dinv, c["itermax"], eps)
    want["dinv"] = dinv
    p = problem(c, tmp)
    assert np.array_equal(p.rhs()[0], b)
    if c["sigma"] > 1:  # the restatement walks the device's own permutation
        assert np.array_equal(p.array("oldToNewPerm"), op.o2n if op.o2n is not None else np.arange(p.nr))
    seen = modes(p)
    if c["matrix"][0] in ("hpcg", "dims"):
        assert seen == [5, 0], seen  # the generated stencil in Sell-64 has row programs: both kernels run
    for mode in seen:
        assert p.use_packed(mode) == mode
        s = handle(p, c, dinv)
        assert s.launches_per_body() == 10
        same(collect(s, s.solve(c["itermax"], eps)), want, (name, mode))
        s.free()
    if c["eps_rel"] > 0.0 and c["precond"] != "scale":
        assert 1 < want["k"] < c["itermax"]  # eps was reached in the middle
    if c["matrix"] == ("dims", 64, 64, 72):
        assert (p.nr + 255) // 256 == 1152  # more than one level-1 value per thread of the scalar step
    p.free(), g.free()


def test_no_preconditioner_is_the_callers_all_ones(gpu, tmp):
    c = cases.CASES["cd16_sell_64_256_none"]
    p = problem(c, tmp)
    eps = 1e-10 * np.sqrt(p.nr)
    a = hostapi.BiCGStab(p)
    b = hostapi.BiCGStab(p, dinv=np.ones(p.nr))
    ga, gb = collect(a, a.solve(150, eps)), collect(b, b.solve(150, eps))
    assert 1 < ga["k"] < 150
    same(ga, gb, "none == ones")
    assert np.array_equal(ga["dinv"], np.ones(p.nr))
    a.free(), b.free(), p.free()


def test_loop_edge_cases(gpu, tmp):
    c = cases.CASES["scaled_cd16_sell_64_256_jacobi"]
    g, op, b, dinv, eps = ref.build_case(c, tmp)
    p = problem(c, tmp)
    full = ref.solve(op, b, dinv, 150, eps)
    full["dinv"] = dinv
    assert 8 < full["k"] < 150
    # itermax = 1 (and 0): the prologue only
    for im in (1, 0):
        s = hostapi.BiCGStab(p, precond="jacobi")
        got = collect(s, s.solve(im, eps))
        want = ref.solve(op, b, dinv, im, eps)
        want["dinv"] = dinv
        same(got, want, ("itermax", im))
        assert got["k"] == 1 and len(got["rr"]) == 1 and len(got["rv"]) == 0 and not got["x"].any()
        s.free()
    # in pieces: 3 + 4 + the rest
    s = hostapi.BiCGStab(p, precond="jacobi")
    s.start(150, eps)
    s.run_iters(3)
    s.run_iters(4)
    s.run_iters(full["k"] - 1 - 7)
    same(collect(s, s.finish()), full, "pieces")
    assert s.loop_ms() > 0.0
    # bodies enqueued well past the exit and past itermax change nothing
    s.start(150, eps)
    for _ in range(30):
        s.run_iters(7)
    same(collect(s, s.finish()), full, "past the exit")
    # the same handle again: another itermax and eps, then the first solve once more
    short = ref.solve(op, b, dinv, 9, 0.0)
    short["dinv"] = dinv
    same(collect(s, s.solve(9, 0.0)), short, "second solve")
    same(collect(s, s.solve(150, eps)), full, "third solve")
    same(collect(s, s.solve(150, eps)), full, "fourth solve")
    s.free()
    p.free(), g.free()


def test_check_residual_and_exact_solution(gpu):
    p = hostapi.Problem("generate", 16, 16, 16, fmt="scs", Cc=64, sigma=256)
    s = hostapi.BiCGStab(p, precond="jacobi")
    k = s.solve(150, 1e-9)
    assert 1 < k < 150
    x = s.solution()
    assert s.check_residual() == np.max(np.abs(x - 1.0)) < 1e-8
    s.free(), p.free()


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
    L.sb_bicgstab_create(m, None, b.ctypes.data_as(hostapi.vp), None, 0, None)
elif what == "sp":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1, precision="single")
    b = np.ones(p.nr)
    L.sb_bicgstab_create(p.matrix, None, b.ctypes.data_as(hostapi.vp), None, 0, None)
elif what == "seq":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    L.sb_set_dot_order(1)
    hostapi.BiCGStab(p)
elif what == "seq_start":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    s = hostapi.BiCGStab(p)
    L.sb_set_dot_order(1)
    s.start(10, 0.0)
elif what in ("zero_diagonal_crs", "zero_diagonal_scs"):
    p = hostapi.Problem(sys.argv[2], 1, 1, 1, fmt=what[-3:], Cc=64, sigma=1)
    hostapi.BiCGStab(p, precond="jacobi")
elif what == "zero_dinv":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    d = -np.ones(p.nr)
    d[37] = 0.0
    hostapi.BiCGStab(p, dinv=d)
elif what == "nan_dinv":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="crs")
    d = np.ones(p.nr)
    d[5] = np.nan
    hostapi.BiCGStab(p, dinv=d)
elif what == "negative_dinv_is_legal":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="crs")
    s = hostapi.BiCGStab(p, dinv=-np.ones(p.nr))
    k = s.solve(5, 0.0)
    assert k == 5 and np.array_equal(s.dinv(), -np.ones(p.nr))
    print("SOLVED")
    sys.exit(0)
print("NOT REFUSED")
"""


def zero_diagonal_file(tmp):
    """a 6 x 6 tridiagonal matrix whose rows 2 and 4 have a 0.0 diagonal (row 4 stores it explicitly, row 2 not at all); the
    other diagonal entries are negative, which BiCGStab's Jacobi takes"""
    path = os.path.join(str(tmp), "zero_diagonal.mtx")
    ent = []
    for i in range(6):
        if i > 0:
            ent.append((i, i - 1, -1.0))
        if i == 4:
            ent.append((i, i, 0.0))
        elif i != 2:
            ent.append((i, i, -4.0))
        if i < 5:
            ent.append((i, i + 1, -1.0))
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write("6 6 %d\n" % len(ent))
        f.write("".join("%d %d %.17g\n" % (r + 1, c + 1, v) for r, c, v in ent))
    return path


def child(what, tmp):
    return subprocess.run([sys.executable, "-c", CHILD % ROOT, what, zero_diagonal_file(tmp)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=300)


@pytest.mark.parametrize("what,msg", [("two_ranks", "BiCGStab runs on one rank (this process is rank 0 of 1, the matrix has 2 halo columns)"),
                                      ("sp", "BiCGStab: double precision only"), ("seq", "tree dot order only"), ("seq_start", "tree dot order only"),
                                      ("zero_diagonal_crs", "2 of 6 matrix rows have no finite non-zero diagonal entry (the first: device row 2)"),
                                      ("zero_diagonal_scs", "2 of 6 matrix rows have no finite non-zero diagonal entry (the first: device row 2)"),
                                      ("zero_dinv", "dinv[37] = 0"), ("nan_dinv", "dinv[5] = nan")])
def test_refusals_end_the_process_with_their_message(gpu, what, msg, tmp):
    """host-side checks: fatal with file:line, exit status 1, no GPU fault"""
    out = child(what, tmp)
    err = out.stderr.decode()
    assert out.returncode == 1, (out.returncode, err[-1000:])
    assert msg in err and "sbhip:" in err and "NOT REFUSED" not in out.stdout.decode(), err[-1000:]
    assert "illegal memory access" not in err and "HIP error" not in err


def test_negative_dinv_entries_are_legal(gpu, tmp):
    out = child("negative_dinv_is_legal", tmp)
    assert out.returncode == 0 and "SOLVED" in out.stdout.decode(), out.stderr.decode()[-1000:]
