"""Restarted GMRES(m) on the GPU against the CPU restatement of its contract (tests/gmres_ref.py): k, the
estimate history, the r.r history and x BIT FOR BIT; the fused kernels == the op list; CRS, Sell-64-1 and Sell-64-256 (the
permuted row order), both SpMV kernel modes; solves in pieces, early exits inside a cycle, the hn ~ 0 path; HPCG 64^3 and
128^3 against the committed golden (made by the restatement on the CPU); and the capability itself: a non-symmetric system
that CG does not solve."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import gmres_cases
import gmres_ref
from conftest import load_json
from sparsebench_amd import hostapi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_REF = {}


def ref(name, tmp):
    if name not in _REF:
        _REF[name] = gmres_ref.run_case(name, tmp)
    return _REF[name]


def problem(name, fmt, sigma, tmp):
    c = gmres_cases.CASES[name]
    if c["kind"] == "cd":
        path = gmres_cases.write_convdiff(os.path.join(str(tmp), "cd_%d_%d_%d.mtx" % c["dims"]), *c["dims"])
        return hostapi.Problem(path, fmt=fmt, Cc=64, sigma=sigma)
    if c["kind"] == "file":
        return hostapi.Problem(c["path"], fmt=fmt, Cc=64, sigma=sigma)
    return hostapi.Problem("generate", *c["dims"], fmt=fmt, Cc=64, sigma=sigma)


def run_gpu(p, m, itermax, eps, fused=True):
    s = hostapi.GMRES(p, restart=m, fused=fused)
    k = s.solve(itermax, eps)
    res, rr = s.history()
    out = dict(k=k, res=res, rr=rr, x=s.solution(), counters=s.counters(), launches=[s.launches_per_step(j) for j in range(m)])
    s.free()
    return out


def same(got, want, what):
    assert got["k"] == want["k"], (what, got["k"], want["k"])
    for key in ("res", "rr", "x"):
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        bad = np.nonzero(a.view(np.uint64) != b.view(np.uint64))[0]
        assert bad.size == 0, (what, key, "first difference at", int(bad[0]), a[bad[0]], b[bad[0]])


SMALL_CD = ["cd16_m30", "cd16_m10", "cd16_m1", "cd_10_11_13_m30", "cd32_m30"]


@pytest.mark.parametrize("fmt", ["crs", "scs"])
@pytest.mark.parametrize("name", SMALL_CD + ["band_klein_eps", "band_klein_eps0"])
def test_bit_identical_to_the_restatement_fused_and_op_list(gpu, name, fmt, tmp_path):
    """convection-diffusion (non-symmetric) as CRS and as Sell-64-1; matrix_band_klein, whose b is an eigenvector: one step
    ends it, and eps = 0 drives it through the hn ~ 0 path -- whatever the contract yields there, both sides yield it"""
    c = gmres_cases.CASES[name]
    want = ref(name, tmp_path)
    p = problem(name, fmt, 1, tmp_path)
    for fused in (True, False):
        got = run_gpu(p, c["m"], c["itermax"], want["eps"], fused)
        same(got, want, (name, fmt, fused))
        m = c["m"]
        assert got["launches"] == ([0] * m if not fused else [7 + (j == 0) + 5 * (j == m - 1) for j in range(m)])
        assert got["counters"]["steps"] == want["k"] - 1 and got["counters"]["n_res"] == len(want["res"])
        assert got["counters"]["cycles"] == len(want["rr"]) - 1
    p.free()
    if name == "band_klein_eps0":
        assert want["k"] == 21 and not np.isnan(want["res"]).any()


@pytest.mark.parametrize("mode", [5, 0])
@pytest.mark.parametrize("name", ["hpcg16_m30", "hpcg32_m30"])
def test_sell_64_256_permuted_order_both_kernel_modes(gpu, name, mode, tmp_path):
    c = gmres_cases.CASES[name]
    want = ref(name, tmp_path)
    p = problem(name, "scs", 256, tmp_path)
    p.use_packed(mode)
    for fused in (True, False):
        same(run_gpu(p, c["m"], c["itermax"], want["eps"], fused), want, (name, mode, fused))
    p.free()


@pytest.mark.parametrize("fused", [True, False])
def test_in_pieces_equals_solve(gpu, fused, tmp_path):
    name = "cd16_m10"
    c = gmres_cases.CASES[name]
    want = ref(name, tmp_path)
    p = problem(name, "scs", 1, tmp_path)
    s = hostapi.GMRES(p, restart=c["m"], fused=fused)
    s.start(c["itermax"], want["eps"])
    for _ in range((c["itermax"] + 6) // 7):  # (steps past the exit are no-ops)
        s.run_steps(7)
    k = s.finish()
    res, rr = s.history()
    same(dict(k=k, res=res, rr=rr, x=s.solution()), want, ("pieces", fused))
    # a solve abandoned with steps outstanding: finish closes the open cycle over the columns it has
    op, b, m, _, eps = gmres_ref.build_case(name, tmp_path)
    short = gmres_ref.solve(op, b, m, 14, eps)  # 13 steps: one full cycle + 3 columns
    s.start(c["itermax"], want["eps"])
    s.run_steps(13)
    s.finish()
    assert np.array_equal(s.solution(), op.to_orig(short["x"]))
    s.free(), p.free()


def test_early_exit_in_the_middle_of_a_cycle(gpu, tmp_path):
    """eps chosen from the golden history so that the loop test trips at cycle position 11 of the first cycle: x carries that
    partial cycle"""
    name = "cd16_m30"
    c = gmres_cases.CASES[name]
    res = gmres_ref.unhex(load_json("gmres_hist.json")["cases"][name]["res"])
    assert res[12] < res[11]
    eps = 0.5 * (res[11] + res[12])  # the step at counter 12 is cycle position 11
    op, b, m, itermax, _ = gmres_ref.build_case(name, tmp_path)
    want = gmres_ref.solve(op, b, m, itermax, eps)
    want["x"] = op.to_orig(want["x"])
    assert want["k"] == 13 and len(want["rr"]) == 2 and want["x"].any()
    p = problem(name, "crs", 1, tmp_path)
    for fused in (True, False):
        same(run_gpu(p, m, itermax, eps, fused), want, ("early", fused))
    p.free()


@pytest.mark.parametrize("name", ["hpcg64_m30", "hpcg128_m30"])
def test_hpcg_64_and_128_against_the_committed_golden(gpu, name):
    """the restatement is too slow to rerun here at 128^3: its run on the CPU is the golden file (k, both histories as exact
    doubles, a SHA-256 of x's bytes); tests/test_gmres_host.py pins the file to the restatement"""
    c = gmres_cases.CASES[name]
    gold = load_json("gmres_hist.json")["cases"][name]
    p = hostapi.Problem("generate", *c["dims"], fmt="scs", Cc=64, sigma=256)
    for fused in (True, False):
        got = run_gpu(p, c["m"], c["itermax"], float.fromhex(gold["eps"]), fused)
        assert got["k"] == gold["k"]
        for key in ("res", "rr"):
            want = gmres_ref.unhex(gold[key])
            assert got[key].shape == want.shape and np.array_equal(got[key].view(np.uint64), want.view(np.uint64)), (name, fused, key)
        assert hashlib.sha256(np.ascontiguousarray(got["x"]).tobytes()).hexdigest() == gold["x_sha256"], (name, fused)
    p.free()


def test_gmres_solves_what_cg_cannot(gpu, tmp_path):
    """the capability this adds, shown once: on the non-symmetric convection-diffusion matrix CG runs to itermax without
    ever getting below its initial residual; GMRES(30) converges to 1e-10 ||b||"""
    name = "cd16_m30"
    c = gmres_cases.CASES[name]
    want = ref(name, tmp_path)
    p = problem(name, "scs", 1, tmp_path)
    s = hostapi.GMRES(p, restart=30)
    k = s.solve(150, want["eps"])
    res, rr = s.history()
    assert k < 150 and res[-1] <= want["eps"] and np.sqrt(rr[-1]) <= 10 * want["eps"]
    s.free()
    cg = hostapi.CG(p)
    assert cg.solve(150, want["eps"]) == 150
    crr, _ = cg.history()
    assert not (np.sqrt(crr[1:]) < np.sqrt(crr[0])).any()
    cg.free(), p.free()


CHILD = r"""
import sys
sys.path.insert(0, %r)
from sparsebench_amd import capi, hostapi
import numpy as np
capi.init(0)
what = sys.argv[1]
if what == "sp":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1, precision="single")
    b = np.ones(p.nr)
    capi.load().sb_gmres_create(p.matrix, None, b.ctypes.data_as(hostapi.vp), None, 30)
else:
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
    hostapi.GMRES(p, restart=0)
print("NOT REFUSED")
"""


@pytest.mark.parametrize("what,msg", [("sp", "GMRES: double precision only"), ("restart0", "restart = 0")])
def test_refusals_end_the_process_with_their_message(gpu, what, msg):
    """host-side argument checks: fatal with file:line before any kernel is launched"""
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT, what], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 1, (out.returncode, out.stderr.decode()[-1000:])
    err = out.stderr.decode()
    assert msg in err and "sbhip:" in err and "NOT REFUSED" not in out.stdout.decode()
