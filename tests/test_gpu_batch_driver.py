"""`-t cg -n <nrhs>` from the benchmark drivers and solveCGBatch from both drop-in libraries (a C caller written against
include/sparsebench/sparsebench.h only), against the CPU restatement of solveCG on every column's right-hand side."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po

import cg_batch_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")
BIN = os.path.join(ROOT, "sparsebench_amd", "bin")
ITERMAX = 60


@pytest.fixture(scope="module")
def want16():
    g = po.GMatrix.generate(16, 16, 16)
    B = ref.batch_rhs(g.rhs(), 4)
    out = [ref.solve(ref.operator(g), B[c], ITERMAX, 0.0) for c in range(4)]
    g.free()
    return out


def run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def check_lines(txt, want, itermax):
    freq = max(1, min(50, itermax // 10))
    for c, w in enumerate(want):
        assert "RHS %d: Initial Residual = %E" % (c, np.sqrt(w["rr"][0])) in txt, c
        for j in range(1, w["k"]):
            if j % freq == 0 or j + 1 == itermax:
                assert "RHS %d: Iteration = %d Residual = %E" % (c, j, np.sqrt(w["rr"][0 if j == 1 else j - 1])) in txt, (c, j)
        assert "RHS %d: Solution performed %d iterations\n" % (c, w["k"]) in txt, c
    assert re.search(r"^Solution performed %d iterations and took \d+\.\d\ds$" % max(w["k"] for w in want), txt, re.M)


@pytest.mark.parametrize("exe", ["sparseBench-CRS-HIP", "sparseBench-SCS-HIP"])
def test_driver_runs_batched_cg(gpu, exe, want16):
    out = run([os.path.join(BIN, exe), "-t", "cg", "-n", "4", "-x", "16", "-y", "16", "-z", "16", "-i", str(ITERMAX)])
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    txt = out.stdout.decode()
    assert "Test type: CG" in txt
    check_lines(txt, want16, ITERMAX)
    assert "Difference between computed and exact  = " in txt
    assert "Function   Rate(MB/s)  Rate(MFlop/s)  Walltime(s)" in txt
    # -n 1 is the single solver's path: no RHS prefix
    one = run([os.path.join(BIN, exe), "-t", "cg", "-n", "1", "-x", "16", "-y", "16", "-z", "16", "-i", str(ITERMAX)])
    none = run([os.path.join(BIN, exe), "-t", "cg", "-x", "16", "-y", "16", "-z", "16", "-i", str(ITERMAX)])
    assert one.returncode == 0 and "RHS" not in one.stdout.decode()

    def solver_lines(t):  # (times and rates vary from run to run)
        return [re.sub(r" and took .*", "", ln) for ln in t.splitlines() if re.match(r"Initial Residual|Iteration =|Solution performed|Test type", ln)]

    assert none.returncode == 0 and solver_lines(one.stdout.decode()) == solver_lines(none.stdout.decode())
    assert len(solver_lines(one.stdout.decode())) >= 4
    assert "Initial Residual = %E" % np.sqrt(want16[0]["rr"][0]) in one.stdout.decode()


def test_driver_refusals(gpu):
    crs = os.path.join(BIN, "sparseBench-CRS-HIP")
    size = ["-x", "8", "-y", "8", "-z", "8", "-i", "10"]
    out = run([crs, "-t", "cg", "-n", "3"] + size)
    assert out.returncode == 1 and "2, 4 or 8" in out.stderr.decode() and "sbhip:" in out.stderr.decode()
    for t in ("spmv", "gmres"):
        out = run([crs, "-n", "2", "-t", t] + size)
        assert out.returncode == 1 and "-t cg only" in out.stderr.decode(), t
    for exe in ("sparseBench-CRS-HIP-SP", "sparseBench-SCS-HIP-SP"):
        out = run([os.path.join(BIN, exe), "-t", "cg", "-n", "4"] + size)
        assert out.returncode == 1 and "batched CG: double precision only" in out.stderr.decode()
    assert "Number of right-hand sides for -t cg. Default 1." in run([crs, "-h"]).stdout.decode()


@pytest.mark.parametrize("fmt", ["CRS", "SCS"])
def test_c_caller_of_solveCGBatch(gpu, fmt, want16, tmp_path):
    exe = os.path.join(str(tmp_path), "batch_driver_%s" % fmt)
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-Wall", "-D" + fmt, "-I" + os.path.join(ROOT, "include"),
                           "-DSOLVER_BATCH", os.path.join(ROOT, "tests", "c", "solver_driver.c"), "-o", exe, "-L" + LIB,
                           "-lsparsebench_%s" % fmt.lower(), "-lsparsebench_host", "-lsbhip", "-Wl,-rpath," + LIB, "-lm"])
    out = run([exe, "16", str(ITERMAX), "0.0", "4"])
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    txt = out.stdout.decode()
    assert int(re.search(r"^k (\d+)$", txt, re.M).group(1)) == max(w["k"] for w in want16)
    check_lines(txt, want16, ITERMAX)
