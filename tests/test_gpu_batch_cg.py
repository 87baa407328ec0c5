"""Batched CG on the GPU.  For every case two equalities hold BIT FOR BIT (k_c, every r.r, every p.Ap, x_c):
column c of the batched solve == sb_cg_create(..., b_c, ...) solved alone in the tree order, with fused = 1 and with
fused = 0; and == the CPU restatement of solveCG (tests/cg_batch_ref.py, pinned to the oracle by tests/test_cg_batch_host.py).
(NaN compares equal to NaN: the numpy restatement's 0/0 carries the sign bit x86 gives it.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po

import cg_batch_ref as ref
from conftest import REFDATA, load_json
from sparsebench_amd import capi, hostapi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = os.path.join(REFDATA, "matrix_band_klein.mtx")


class SingleCG(hostapi.CG):
    """hostapi.CG on a right-hand side of the caller's, in the tree order"""

    def __init__(self, problem, b, fused):
        self.L = capi.load()
        self.problem = problem
        self.single = False
        b = np.ascontiguousarray(b, dtype=np.float64)
        self.ptr = self.L.sb_cg_create(problem.matrix, problem.halo, b.ctypes.data_as(hostapi.vp), None)
        self.L.sb_cg_set_fused(self.ptr, int(fused))
        self.L.sb_cg_set_dot_order(self.ptr, 0)
        self.itermax = 0


def solve_single(p, b, itermax, eps, fused):
    s = SingleCG(p, b, fused)
    k = s.solve(itermax, eps)
    rr, pAp = s.history()
    out = dict(k=k, rr=rr, pAp=pAp, x=s.solution())
    s.free()
    return out


def collect(s):
    out = []
    for c in range(s.nrhs):
        rr, pAp = s.history(c)
        out.append(dict(k=s.iterations(c), rr=rr, pAp=pAp, x=s.solution(c)))
    return out


def solve_batch(p, B, itermax, eps):
    s = hostapi.BatchCG(p, B)
    kmax = s.solve(itermax, eps)
    cols = collect(s)
    assert kmax == max(c["k"] for c in cols)
    assert s.counters()["all_stopped"] == 1 and s.counters()["columns_stopped"] == s.nrhs
    s.free()
    return cols


def same(got, want, what):
    assert got["k"] == want["k"], (what, "k", got["k"], want["k"])
    for key in ("rr", "pAp", "x"):
        a, b = np.ascontiguousarray(got[key], dtype=np.float64), np.ascontiguousarray(want[key], dtype=np.float64)
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        na, nb = np.isnan(a), np.isnan(b)
        assert np.array_equal(na, nb), (what, key, "NaN positions differ")
        bad = np.nonzero((a.view(np.uint64) != b.view(np.uint64)) & ~na)[0]
        assert bad.size == 0, (what, key, "first difference at", int(bad[0]), a[bad[0]], b[bad[0]])


def check_all(p, op, B, itermax, eps, what, fused_levels=(1, 0)):
    """the two equalities for every column; returns the restatement's results"""
    cols = solve_batch(p, B, itermax, eps)
    wants = []
    for c in range(len(B)):
        want = ref.solve(op, B[c], itermax, eps)
        wants.append(want)
        same(cols[c], want, (what, "restatement", c))
        for fused in fused_levels:
            same(cols[c], solve_single(p, B[c], itermax, eps, fused), (what, "single fused=%d" % fused, c))
    return wants


def generated(dims, fmt, Cc, sigma):
    p = hostapi.Problem("generate", *dims, fmt=fmt, Cc=Cc, sigma=sigma)
    g = po.GMatrix.generate(*dims)
    op = ref.operator(g, fmt, Cc, sigma)
    if sigma > 1:  # the restatement walks the device's own permutation
        assert np.array_equal(p.array("oldToNewPerm"), op.o2n if op.o2n is not None else np.arange(p.nr))
    return p, g, op


CASES = {"sell_64_1_16": ((16, 16, 16), "scs", 64, 1, 60), "sell_64_256_32": ((32, 32, 32), "scs", 64, 256, 60),
         "crs_16": ((16, 16, 16), "crs", 64, 1, 60), "sell_4_8_8": ((8, 8, 8), "scs", 4, 8, 30),
         "sell_64_256_10_11_13": ((10, 11, 13), "scs", 64, 256, 60)}


@pytest.mark.parametrize("nv", [2, 4, 8])
@pytest.mark.parametrize("case", list(CASES))
def test_every_column_is_the_single_solve_and_the_restatement(gpu, case, nv):
    dims, fmt, Cc, sigma, itermax = CASES[case]
    p, g, op = generated(dims, fmt, Cc, sigma)
    b0, xe = p.rhs()
    assert np.array_equal(b0, g.rhs())
    B = ref.batch_rhs(b0, nv)
    s = hostapi.BatchCG(p, nrhs=nv)  # B = None: the rule, computed by the library's side
    assert s.launches_per_body() == (5 if (fmt == "scs" and Cc == 64) else 6)
    s.solve(itermax, 0.0)
    rule = collect(s)
    resid = s.check_residual(0)
    assert s.check_residual(1) == 0.0  # no exact solution for c >= 1
    s.free()
    wants = check_all(p, op, B, itermax, 0.0, (case, nv))
    for c in range(nv):
        same(rule[c], wants[c], (case, nv, "B=None", c))
    one = hostapi.CG(p, dot_order="tree")
    one.solve(itermax, 0.0)
    assert resid == one.check_residual()
    one.free(), p.free(), g.free()


@pytest.mark.parametrize("nv", [2, 4, 8])
def test_columns_that_stop_at_different_iterations(gpu, nv):
    """b_c = b_0 * 2^(-10 c) scales every column's residuals by an exact power of two; with one eps > 0 the columns leave
    the loop at different k -- the restatement says which -- and a column that has left no longer changes"""
    p, g, op = generated((16, 16, 16), "scs", 64, 1)
    b0, _ = p.rhs()
    B = np.stack([b0 * 2.0 ** (-10 * c) for c in range(nv)])
    eps = float(np.sqrt(po.ddot_tree(b0, b0))) * 2.0 ** -25
    wants = check_all(p, op, B, 150, eps, ("stops", nv))
    ks = [w["k"] for w in wants]
    assert len(set(ks[:4])) == len(ks[:4]) and max(ks) < 150, ks  # columns 0 .. 3 all differ (from column 3 on, k = 1)
    assert ks[0] == max(ks)
    p.free(), g.free()


def test_a_zero_column(gpu):
    p, g, op = generated((16, 16, 16), "scs", 64, 1)
    b0, _ = p.rhs()
    B = ref.batch_rhs(b0, 4)
    B[2] = 0.0
    wants = check_all(p, op, B, 40, 0.0, "zero column")
    assert wants[2]["k"] == 1 and not wants[2]["x"].any() and wants[0]["k"] == 40
    p.free(), g.free()


@pytest.mark.parametrize("fmt", ["crs", "scs"])
def test_band_klein_nan_exit_beside_columns_that_run_on(gpu, fmt):
    """matrix_band_klein with initVectors' b: the loop leaves at k = 3 on a NaN residual; the other columns iterate on"""
    p = hostapi.Problem(BAND, 1, 1, 1, fmt=fmt, Cc=64, sigma=1)
    g = po.GMatrix.from_mtx(BAND)
    op = ref.operator(g, fmt, 64, 1)
    b0, xe = p.rhs()
    assert xe is None and np.array_equal(b0, g.rhs())
    B = ref.batch_rhs(b0, 4)
    wants = check_all(p, op, B, 30, 0.0, ("band_klein", fmt))
    assert wants[0]["k"] == 3 and max(w["k"] for w in wants[1:]) > 3
    p.free(), g.free()


def test_itermax_one(gpu):
    p, g, op = generated((16, 16, 16), "scs", 64, 1)
    B = ref.batch_rhs(p.rhs()[0], 4)
    wants = check_all(p, op, B, 1, 0.0, "itermax 1")
    assert all(w["k"] == 1 and len(w["rr"]) == 1 and len(w["pAp"]) == 0 for w in wants)
    p.free(), g.free()


def test_in_pieces_and_the_same_handle_twice(gpu):
    p, g, op = generated((16, 16, 16), "scs", 64, 256)
    b0, _ = p.rhs()
    B = np.stack([b0 * 2.0 ** (-10 * c) for c in range(4)])
    eps = float(np.sqrt(po.ddot_tree(b0, b0))) * 2.0 ** -25
    wants = [ref.solve(op, B[c], 150, eps) for c in range(4)]
    s = hostapi.BatchCG(p, B)
    s.start(150, eps)
    for _ in range(30):  # 210 bodies: well past every column's exit, and past itermax
        s.run_iters(7)
    assert s.finish() == max(w["k"] for w in wants)
    assert s.counters()["bodies_enqueued"] == 210 and s.loop_ms() > 0.0
    for c, got in enumerate(collect(s)):
        same(got, wants[c], ("pieces", c))
    # the same handle again: another itermax and eps, then the first solve once more
    short = [ref.solve(op, B[c], 9, 0.0) for c in range(4)]
    assert s.solve(9, 0.0) == 9
    for c, got in enumerate(collect(s)):
        same(got, short[c], ("second solve", c))
    s.solve(150, eps)
    for c, got in enumerate(collect(s)):
        same(got, wants[c], ("third solve", c))
    s.free(), p.free(), g.free()


@pytest.mark.parametrize("key", ["hpcg64_x1_scs_C64_sigma1", "hpcg128_x1_scs_C64_sigma256"])
def test_hpcg_64_and_128_against_the_committed_golden(gpu, key):
    """column 0 == the committed tree-order history (tests/golden/cg_hist_tree.json, made by the oracle on the CPU); the
    other columns == single solves on the same device"""
    e = load_json("cg_hist_tree.json")[key]
    n = e["n"]
    p = hostapi.Problem("generate", n, n, n, fmt="scs", Cc=e["C"], sigma=e["sigma"])
    B = ref.batch_rhs(p.rhs()[0], 4)
    cols = solve_batch(p, B, e["itermax"], 0.0)
    assert cols[0]["k"] == e["k"]
    assert ref.same_bits(cols[0]["rr"], np.array([float(v) for v in e["rr"]]))
    assert ref.same_bits(cols[0]["pAp"], np.array([float(v) for v in e["pAp"]]))
    for c in range(4):
        for mode in ((0, 5) if c == 1 else (5,)):  # one column against both single-vector kernels
            p.use_packed(mode)
            same(cols[c], solve_single(p, B[c], e["itermax"], 0.0, 1), (key, "single", c, mode))
    p.free()


CHILD = r"""
import sys
sys.path.insert(0, %r)
from sparsebench_amd import capi, hostapi
import numpy as np
L = capi.init(0)
what = sys.argv[1]
if what == "sp":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1, precision="single")
    B = np.ones((4, p.nr))
    L.sb_cgb_create(p.matrix, None, 4, B.ctypes.data_as(hostapi.vp), None)
elif what == "seq":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    L.sb_set_dot_order(1)
    hostapi.BatchCG(p, nrhs=4)
elif what == "seq_start":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    s = hostapi.BatchCG(p, nrhs=4)
    L.sb_set_dot_order(1)
    s.start(10, 0.0)
else:
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    hostapi.BatchCG(p, nrhs=int(what))
print("NOT REFUSED")
"""


@pytest.mark.parametrize("what,msg", [("sp", "double precision only"), ("seq", "tree dot order only"), ("seq_start", "tree dot order only"),
                                      ("3", "2, 4 or 8"), ("1", "sb_cg_create"), ("16", "2, 4 or 8")])
def test_refusals_end_the_process_with_their_message(gpu, what, msg):
    """host-side argument checks: fatal with file:line before any kernel is launched"""
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT, what], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 1, (out.returncode, out.stderr.decode()[-1000:])
    err = out.stderr.decode()
    assert msg in err and "sbhip:" in err and "NOT REFUSED" not in out.stdout.decode()
