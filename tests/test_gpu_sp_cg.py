"""Single-precision CG on the MI355X: the reference's own SP solveCG history (tests/golden/cg_hist_sp_ref.json) bit for bit in
the seq order, the fused tree-order loop against the unfused op list and against tests/sp_ref.py, the exact r.r = 0 exit of
HPCG 8^3, the SP drivers, and an SP solve followed by a DP solve in one process."""
import json
import os
import subprocess

import numpy as np
import pytest

import sp_ref
from sparsebench_amd import capi, hostapi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BAND = os.path.join(GOLDEN, "ref", "matrix_band_klein.mtx")
BIN = os.path.join(ROOT, "sparsebench_amd", "bin")
F = np.float32


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.init(0)


def golden(name, which="cg_hist_sp_ref.json"):
    return json.load(open(os.path.join(GOLDEN, which)))[name]


def problem(name, fmt, Cc=64, sigma=1, precision="single"):
    if name == "band_klein":
        return hostapi.Problem(BAND, 1, 1, 1, fmt=fmt, Cc=Cc, sigma=sigma, precision=precision)
    n = int(name[4:])
    return hostapi.Problem("generate", n, n, n, fmt=fmt, Cc=Cc, sigma=sigma, precision=precision)


def bits(a):
    a = np.asarray(a, F)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def solve(p, itermax, order, fused=True):
    cg = hostapi.CG(p, fused=fused, dot_order=order)
    k = cg.solve(itermax)
    rr, pap = cg.history()
    x = cg.solution()
    cg.free()
    return k, rr, pap, x


CASES = [(n, f, c, s) for n in ("band_klein", "hpcg8", "hpcg16", "hpcg32", "hpcg64")
         for (f, c, s) in (("crs", 64, 1), ("scs", 64, 1), ("scs", 64, 256))] + [("hpcg128", "scs", 64, 256)]


@pytest.mark.parametrize("name,fmt,Cc,sigma", CASES)
def test_seq_history_is_the_references(name, fmt, Cc, sigma):
    g = golden(name)
    p = problem(name, fmt, Cc, sigma)
    k, rr, pap, x = solve(p, g["itermax"], "seq")
    assert x.dtype == np.float32
    assert k == g["k"]
    assert np.array_equal(bits(rr), bits([float(v) for v in g["rr"]])), name
    assert np.array_equal(bits(pap), bits([float(v) for v in g["pAp"]])), name
    p.free()


def test_hpcg8_exits_on_exact_zero():
    """r.r underflows to exactly 0 on the way through f32 subnormals: normr = 0 fails `normr > eps` and the loop ends at k = 44"""
    p = problem("hpcg8", "crs")
    for order in ("seq", "tree"):
        k, rr, pap, _ = solve(p, 150, order)
        assert rr[-1] == 0.0 and k == len(rr) + 1, (order, k)
        if order == "seq":
            assert k == 44
    p.free()


@pytest.mark.parametrize("name,fmt,sigma", [("hpcg8", "crs", 1), ("hpcg16", "crs", 1), ("hpcg8", "scs", 1), ("hpcg16", "scs", 1),
                                            ("hpcg16", "scs", 256), ("band_klein", "scs", 1)])
def test_tree_fused_equals_op_list_and_sp_ref(name, fmt, sigma):
    p = problem(name, fmt, 64, sigma)
    itermax = 150
    a = solve(p, itermax, "tree", fused=True)
    b = solve(p, itermax, "tree", fused=False)
    assert a[0] == b[0]
    for u, v in zip(a[1:], b[1:]):
        assert np.array_equal(bits(u), bits(v))
    cg = hostapi.CG(p, dot_order="tree")
    assert cg.launches_per_body() == (3 if fmt == "scs" else 4)
    cg.set_dot_order("seq")
    assert cg.launches_per_body() == 0
    cg.free()
    if sigma == 1:  # the tree runs over the device's row order: the original one
        c = problem(name, "crs")
        rp, col, val = c.array("rowPtr"), c.array("crs_colInd"), c.values()
        bvec, _ = c.rhs()
        k, rr, pap, x = sp_ref.cg(lambda v: sp_ref.spmv_crs(rp, col, val, v), bvec, itermax)
        assert a[0] == k
        assert np.array_equal(bits(a[1]), bits(rr)) and np.array_equal(bits(a[2]), bits(pap))
        assert np.array_equal(bits(a[3]), bits(x))
        c.free()
    p.free()


def test_sp_then_dp_in_one_process():
    """an SP solve, then the DP path: the DP reference history (cg_hist_1rank.json) unchanged"""
    p = problem("hpcg16", "scs", 64, 256)
    solve(p, 150, "seq")
    p.free()
    g = golden("hpcg8", "cg_hist_1rank.json")
    q = problem("hpcg8", "crs", precision="double")
    k, rr, pap, x = solve(q, g["itermax"], "seq")
    assert x.dtype == np.float64 and k == g["k"]
    assert np.array_equal(rr, np.array([float(v) for v in g["rr"]]))
    assert np.array_equal(pap, np.array([float(v) for v in g["pAp"]]))
    q.free()


def _expected_lines(name, itermax):
    """the lines the reference's SP solveCG prints (src/CGSolver.c:101,118-120,132-135) from its recorded history"""
    g = golden(name)
    rr = [float(v) for v in g["rr"]]
    freq = min(max(itermax // 10, 1), 50)
    out = ["Initial Residual = %E" % F(np.sqrt(rr[0]))]
    for j in range(1, g["k"]):
        if j % freq == 0 or j + 1 == itermax:
            out.append("Iteration = %d Residual = %E" % (j, F(np.sqrt(rr[0 if j == 1 else j - 1]))))
    out.append("Solution performed %d iterations" % g["k"])
    return out


@pytest.mark.parametrize("fmt", ["CRS", "SCS"])
def test_sp_driver_prints_the_references_lines(fmt):
    exe = os.path.join(BIN, "sparseBench-%s-HIP-SP" % fmt)
    env = dict(os.environ, SB_DOT_ORDER="seq")
    r = subprocess.run([exe, "-x", "16", "-y", "16", "-z", "16", "-i", "150"], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "single precision floats" in r.stdout
    lines = r.stdout.splitlines()
    for want in _expected_lines("hpcg16", 150):
        assert any(l.startswith(want) for l in lines), (want, r.stdout[-3000:])


def test_sp_driver_spmv_through_the_hook():
    """-t spmv: the reference's loop over vectors from allocate(); the SP kernels run in place"""
    exe = os.path.join(BIN, "sparseBench-SCS-HIP-SP")
    env = dict(os.environ, SB_COPY_REPORT="1")
    r = subprocess.run([exe, "-t", "spmv", "-x", "32", "-y", "32", "-z", "32", "-i", "20"], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "single precision floats" in r.stdout and "Test type: SPMVM" in r.stdout
    row = [l for l in r.stdout.splitlines() if l.startswith("spMVM:")]
    assert row and float(row[0].split()[1]) > 0.0, r.stdout[-2000:]  # MB/s of the device-timed spMVM regions
