"""The reference's own dot order on the GPU (sb_set_dot_order(1) / SB_DOT_ORDER=seq / CG(dot_order="seq")): one
sequential sum per rank in original row order, every product rounded before its add (src/solver.c:41-62 as shipped).
With it the GPU gives the reference's numbers bit for bit -- the dot against the oracle's orc_ddot_seq, solveCG against
the oracle's seq-order CG and against the histories captured from the reference itself (tests/golden) -- where the
default tree order is only within the sequential sum's own rounding error of them."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REFDATA, load_json
from oracle import pyoracle as po
from sparsebench_amd import capi, hostapi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")
CONFIGS = [("crs", 64, 1), ("scs", 64, 1), ("scs", 64, 256), ("scs", 4, 1), ("scs", 128, 512)]


def f(a):
    return np.array([float(v) for v in a])


def adversarial(n, seed):
    """products spanning 40 orders of magnitude with both signs: the sequential and the tree sum round differently"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * np.exp2(rng.integers(-60, 60, n))
    y = rng.standard_normal(n)
    return x, y


def discriminating(n):
    for seed in range(1000):
        x, y = adversarial(n, seed)
        if po.ddot_seq(x, y) != po.ddot_tree(x, y):
            return x, y
    raise AssertionError("no vectors of length %d where the two orders differ" % n)


def gpu_dot(L, x, y):
    a, b = capi.DeviceVector.from_host(x), capi.DeviceVector.from_host(y)
    try:
        return L.sb_ddot(len(x), a.ptr, b.ptr)
    finally:
        a.free(), b.free()


@pytest.fixture
def seq_default(gpu):
    """the process default set to seq for one test, and back to tree whatever happens"""
    assert gpu.sb_dot_order() == 0
    gpu.sb_set_dot_order(1)
    try:
        yield gpu
    finally:
        gpu.sb_set_dot_order(0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 2 ** 20 + 3])
def test_sb_ddot_seq_is_the_sequential_sum(gpu, n):
    x, y = (adversarial(1, 0) if n == 1 else discriminating(n))
    seq, tree = po.ddot_seq(x, y), po.ddot_tree(x, y)
    assert n == 1 or seq != tree  # (one element: both orders are the one product)
    assert gpu.sb_dot_order() == 0 and gpu_dot(gpu, x, y) == tree  # the default is still the tree order
    gpu.sb_set_dot_order(1)
    try:
        assert gpu.sb_dot_order() == 1
        got = gpu_dot(gpu, x, y)
    finally:
        gpu.sb_set_dot_order(0)
    assert got == seq, (n, got, seq, tree)
    assert gpu_dot(gpu, x, y) == tree


def test_sb_ddot_seq_special_values(seq_default):
    L = seq_default
    x, y = adversarial(1000, 5)
    x[500] = np.inf
    got = gpu_dot(L, x, y)
    assert got == po.ddot_seq(x, y) and np.isinf(got)
    x[700] = -np.inf
    y[700] = abs(y[700])
    y[500] = abs(y[500])
    assert np.isnan(gpu_dot(L, x, y)) and np.isnan(po.ddot_seq(x, y))
    z = np.zeros(5)
    got = gpu_dot(L, -z, z)  # (-0.0) * 0.0 = -0.0 five times: the sum starts from +0.0 and stays +0.0
    assert got == 0.0 and not np.signbit(got) and not np.signbit(po.ddot_seq(-z, z))
    assert gpu_dot(L, np.zeros(0), np.zeros(0)) == 0.0


def run_seq(filename, dims, fmt, Cc, sigma, itermax, **kw):
    nx, ny, nz = dims
    p = hostapi.Problem(filename, nx, ny, nz, fmt=fmt, Cc=Cc, sigma=sigma)
    cg = hostapi.CG(p, dot_order="seq", **kw)
    assert cg.dot_order() == "seq" and cg.launches_per_body() == 0 and cg.fuse_p() == 0
    k = cg.solve(itermax, 0.0)
    rr, pap = cg.history()
    out = dict(k=k, rr=rr, pAp=pap, x=cg.solution(), err=cg.check_residual(), regions=cg.region_ms())
    cg.free(), p.free()
    return out


@pytest.mark.parametrize("fmt,Cc,sigma", CONFIGS)
@pytest.mark.parametrize("n", [8, (16, 12, 10), 32])
def test_cg_seq_bit_identical_to_oracle_seq(gpu, fmt, Cc, sigma, n):
    dims = n if isinstance(n, tuple) else (n, n, n)
    o = po.cg(po.GMatrix.generate(*dims), itermax=60, fmt=fmt, Cc=Cc, sigma=sigma, dot="seq", want_x=True)
    r = run_seq("generate", dims, fmt, Cc, sigma, 60)
    assert r["k"] == o["k"]
    assert np.array_equal(r["rr"], o["rr"]) and np.array_equal(r["pAp"], o["pAp"])
    assert np.array_equal(r["x"], o["x"][0])
    assert r["err"] == o["max_err"]
    assert r["regions"]["ddot"] > 0.0  # the reference's op list runs: its region table is filled


REF_CASES = ["band_klein", "hpcg8", "hpcg16", "hpcg32", "hpcg64", "hpcg128"]


@pytest.mark.parametrize("fmt,sigma", [("crs", 1), ("scs", 1), ("scs", 256)])
@pytest.mark.parametrize("name", REF_CASES)
def test_cg_seq_reproduces_the_reference_history(gpu, golden_1rank, name, fmt, sigma):
    """the reference's strict-IEEE solveCG (tests/golden/cg_hist_1rank.json), bit for bit -- also for Sell-64-256, the
    headline layout, whose vectors are stored in permuted order.  Fails in the tree order (2.5e-11 away at 64^3)."""
    gd = golden_1rank[name]
    if name == "band_klein":
        filename, dims = os.path.join(REFDATA, "matrix_band_klein.mtx"), (1, 1, 1)
    else:
        n = int(name[4:])
        filename, dims = "generate", (n, n, n)
    r = run_seq(filename, dims, fmt, 64, sigma, gd["itermax"])
    assert r["k"] == gd["k"]
    assert np.array_equal(r["rr"], f(gd["rr"])), (name, fmt, sigma)
    assert np.array_equal(r["pAp"], f(gd["pAp"])), (name, fmt, sigma)


@pytest.mark.parametrize("name,fmt", [("irregular12", "crs"), ("irregular12", "scs"), ("irregular24", "crs"),
                                      ("irregular24", "scs"), ("irregular80", "crs")])
def test_cg_seq_reproduces_the_reference_on_the_irregular_stand_in(gpu, name, fmt):
    """the reference's own solveCG on the irregular stand-in (tests/golden/cg_hist_irregular_ref.json), bit for bit: at
    80^3 nodes this replaces the tree order's 8.8e-13 against north_star's 1e-12 by equality"""
    e = load_json("cg_hist_irregular_ref.json")[name]
    n = e["nodes_per_edge"]
    r = run_seq("irregular", (n, n, n), fmt, 64, 1, e["itermax"])
    assert r["k"] == e["k"]
    assert np.array_equal(r["rr"], f(e["rr"])) and np.array_equal(r["pAp"], f(e["pAp"])), name


def _solve(cg, itermax=40):
    k = cg.solve(itermax, 0.0)
    rr, pap = cg.history()
    return k, rr, pap, cg.solution()


def test_switching_the_order_on_one_solver(gpu):
    """tree -> seq -> tree on ONE sb_cg: the tree bits, the seq bits, the tree bits; launches_per_body says what runs; the
    caller's fused wishes survive seq; an order asked for inside a solve waits for the next sb_cg_start"""
    dims = (24, 20, 16)
    g = po.GMatrix.generate(*dims)
    ot = po.cg(g, itermax=40, fmt="scs", Cc=64, sigma=256, dot="tree", want_x=True)
    os_ = po.cg(g, itermax=40, fmt="scs", Cc=64, sigma=256, dot="seq", want_x=True)
    assert not np.array_equal(ot["rr"], os_["rr"])  # the two orders are told apart
    p = hostapi.Problem("generate", *dims, fmt="scs", Cc=64, sigma=256)
    cg = hostapi.CG(p)
    assert cg.dot_order() == "tree"
    default_launches, default_fusep = cg.launches_per_body(), cg.fuse_p()
    assert default_launches > 0
    for order, o, launches in (("tree", ot, default_launches), ("seq", os_, 0), ("tree", ot, default_launches),
                               ("seq", os_, 0), (None, ot, default_launches)):
        cg.set_dot_order(order)
        assert cg.dot_order() == ("seq" if order == "seq" else "tree")
        assert cg.launches_per_body() == launches and cg.fuse_p() == (0 if order == "seq" else default_fusep)
        k, rr, pap, x = _solve(cg)
        assert k == o["k"] and np.array_equal(rr, o["rr"]) and np.array_equal(pap, o["pAp"]) and np.array_equal(x, o["x"][0]), order
    # the reference's op list asked for under tree stays asked for across a seq solve
    cg.L.sb_cg_set_fused(cg.ptr, 0)
    cg.set_dot_order("seq")
    assert _solve(cg)[1].tolist() == os_["rr"].tolist()
    cg.set_dot_order("tree")
    assert cg.launches_per_body() == 0
    k, rr, pap, x = _solve(cg)
    assert np.array_equal(rr, ot["rr"]) and np.array_equal(x, ot["x"][0])
    cg.L.sb_cg_set_fused(cg.ptr, 1)
    assert cg.launches_per_body() == default_launches
    # latched per solve: a change between start and finish applies to the next solve only
    for first, second in (("tree", "seq"), ("seq", "tree")):
        cg.set_dot_order(first)
        cg.start(40)
        cg.run_iters(10)
        cg.set_dot_order(second)
        assert cg.dot_order() == first
        cg.L.sb_cg_set_fused(cg.ptr, 1)  # (a fused wish inside a seq solve does not change its op list either)
        cg.run_iters(29)
        k = cg.finish()
        rr, pap = cg.history()
        o = ot if first == "tree" else os_
        assert k == o["k"] and np.array_equal(rr, o["rr"]) and np.array_equal(pap, o["pAp"]), first
        assert cg.dot_order() == second
    cg.free(), p.free()


def test_process_default_and_graph_request(seq_default):
    """a solver without an order of its own follows the process default; a hipGraph request (accepted and ignored: graph
    replay was removed) gives the same bits"""
    g = po.GMatrix.generate(16, 16, 16)
    o = po.cg(g, itermax=50, fmt="scs", Cc=64, sigma=1, dot="seq")
    p = hostapi.Problem("generate", 16, 16, 16, fmt="scs", Cc=64, sigma=1)
    for graph in (False, True):
        cg = hostapi.CG(p, graph=graph)
        assert cg.dot_order() == "seq"
        k, rr, pap, _ = _solve(cg, 50)
        assert k == o["k"] and np.array_equal(rr, o["rr"]) and np.array_equal(pap, o["pAp"]), graph
        cg.set_dot_order("tree")  # the solver's own order beats the process default
        k, rr, pap, _ = _solve(cg, 50)
        assert np.array_equal(rr, po.cg(g, itermax=50, fmt="scs", Cc=64, sigma=1, dot="tree")["rr"])
        cg.free()
    p.free()


CALLER = r"""
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sparsebench/sparsebench.h"

int main(int argc, char** argv)
{
  Comm comm;
  Parameter param;
  commInit(&comm, argc, argv);
  initParameter(&param);
  param.nx = param.ny = param.nz = 32;
  param.itermax = 150;
  const CG_UINT n = 1000;
  CG_FLOAT* x = (CG_FLOAT*)allocate(ARRAY_ALIGNMENT, n * sizeof(CG_FLOAT));
  CG_FLOAT* y = (CG_FLOAT*)allocate(ARRAY_ALIGNMENT, n * sizeof(CG_FLOAT));
  for (CG_UINT i = 0; i < n; i++) {
    x[i] = ldexp((i % 3 ? 1.0 : -1.0) * (1.0 + 0.1 * (double)(i % 7)), (int)((i * 37u) % 121u) - 60);
    y[i] = 1.0 + 1e-3 * (double)(i % 11);
    printf("xy %a %a\n", x[i], y[i]);
  }
  CG_FLOAT d = 0.0;
  ddot(n, x, y, &d);
  printf("dot %a\n", d);
  GMatrix m;
  matrixGenerate(&m, &param, comm.rank, comm.size, false);
  commPartition(&comm, &m);
  Matrix sm;
  memset(&sm, 0, sizeof sm);
#ifdef SCS
  sm.C = 64, sm.sigma = 256;
#endif
  convertMatrix(&sm, &m);
  size_t ff[NUMREGIONS] = { 0 }, fw[NUMREGIONS] = { 0 };
  ff[DDOT] = ff[WAXPBY] = m.totalNr, fw[DDOT] = fw[WAXPBY] = sizeof(CG_FLOAT) * (size_t)m.totalNr;
  ff[SPMVM] = m.totalNnz, fw[SPMVM] = 12 * (size_t)m.totalNnz;
  profilerInit(ff, fw);
  int k = solveCG(&comm, &param, &sm);
  printf("k %d\n", k);
  profilerPrint(&comm, k);
  profilerFinalize();
  commFinalize(&comm);
  return EXIT_SUCCESS;
}
"""


def _residual_lines_match(txt, rr, k):
    assert "Initial Residual = %E" % np.sqrt(rr[0]) in txt
    printed = re.findall(r"^Iteration = (\d+) Residual = (\S+)$", txt, re.M)
    assert len(printed) >= 10
    for it, val in printed:
        j = int(it)
        assert val == "%E" % np.sqrt(rr[0 if j == 1 else j - 1]), (j, val)
    assert "Solution performed %d iterations" % k in txt


@pytest.mark.parametrize("fmt", ["CRS", "SCS"])
def test_reference_shaped_library_follows_the_environment(gpu, golden_1rank, fmt, tmp_path):
    """the drop-in ddot() and solveCG() follow SB_DOT_ORDER: seq gives orc_ddot_seq's bits and the reference's residual
    lines (hpcg32, the golden history), unset the tree order's bits"""
    src = tmp_path / "caller.c"
    src.write_text(CALLER)
    exe = str(tmp_path / ("caller_%s" % fmt))
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-D" + fmt, "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L" + LIB, "-lsparsebench_%s" % fmt.lower(), "-lsparsebench_host", "-lsbhip",
                           "-Wl,-rpath," + LIB, "-lm"], timeout=120)
    gd = golden_1rank["hpcg32"]
    rr = f(gd["rr"])
    for order in ("seq", None):
        env = dict(os.environ)
        env.pop("SB_DOT_ORDER", None)
        if order:
            env["SB_DOT_ORDER"] = order
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        txt = out.stdout.decode()
        pairs = re.findall(r"^xy (\S+) (\S+)$", txt, re.M)
        assert len(pairs) == 1000
        # (contiguous arrays: the oracle reads raw pointers)
        x, y = np.array([float.fromhex(a) for a, _ in pairs]), np.array([float.fromhex(b) for _, b in pairs])
        d = float.fromhex(re.search(r"^dot (\S+)$", txt, re.M).group(1))
        seq, tree = po.ddot_seq(x, y), po.ddot_tree(x, y)
        assert seq != tree
        assert d == (seq if order == "seq" else tree), order
        assert int(re.search(r"^k (\d+)$", txt, re.M).group(1)) == gd["k"]
        if order == "seq":
            _residual_lines_match(txt, rr, gd["k"])
            ddot_row = re.search(r"^ddot:\s+(.*)$", txt, re.M)
            assert ddot_row and float(ddot_row.group(1).split()[0]) > 0.0, txt[-1500:]  # the per-region table of the op list


@pytest.mark.parametrize("fmt", ["CRS", "SCS"])
def test_reference_main_with_seq_prints_the_reference_lines(gpu, golden_1rank, fmt):
    """oracle/_ref/refmain_<FMT>_hip (the reference's src/main.c unchanged, linked with the drop-in) with SB_DOT_ORDER=seq"""
    exe = os.path.join(ROOT, "oracle", "_ref", "refmain_%s_hip" % fmt)
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/refmain_%s_hip was not built (needs /root/reference in the build container)" % fmt)
    gd = golden_1rank["hpcg32"]
    env = dict(os.environ, SPARSEBENCH_C="64", SPARSEBENCH_SIGMA="128", SB_DOT_ORDER="seq")
    out = subprocess.run([exe, "-x", "32", "-y", "32", "-z", "32", "-i", "150"], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300, env=env)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    _residual_lines_match(out.stdout.decode(), f(gd["rr"]), gd["k"])


def test_bad_environment_value_ends_a_gpu_process(gpu):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from sparsebench_amd import capi\n"
            "L = capi.init(0)\n"
            "L.sb_ddot(0, None, None)\n") % ROOT
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SB_DOT_ORDER="kahan"), stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=120)
    assert out.returncode != 0 and "SB_DOT_ORDER=kahan" in out.stderr.decode()
