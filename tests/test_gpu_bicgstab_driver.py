"""`-t bicgstab` from the benchmark drivers and solveBiCGStab from both drop-in libraries (a C caller written against
include/sparsebench/sparsebench.h only), against the CPU restatement of the BiCGStab contract (tests/bicgstab_ref.py) with the
Jacobi preconditioner: on convection-diffusion 16^3 from a Matrix Market file and on the generated 16^3 stencil."""
import os
import re
import subprocess

import numpy as np
import pytest

import bicgstab_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")
BIN = os.path.join(ROOT, "sparsebench_amd", "bin")
ITERMAX = 150
EPS = 1e-9


@pytest.fixture(scope="module")
def wants(tmp_path_factory):
    """restatement runs in the drivers' formats: CRS and Sell-64-1 (the same order: sigma = 1)"""
    tmp = tmp_path_factory.mktemp("bicgstab_driver")
    out = {"path": ref.matrix_path(("cd", 16, 16, 16), tmp)}
    for key, matrix in (("cd", ("cd", 16, 16, 16)), ("hpcg", ("hpcg", 16))):
        g = ref.gmatrix(matrix, tmp)
        out[key] = ref.solve(ref.operator(g), g.rhs(), ref.jacobi(g), ITERMAX, EPS)
        assert 1 < out[key]["k"] < ITERMAX
        g.free()
    return out


def run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def check_lines(txt, w, itermax):
    freq = max(1, min(50, itermax // 10))
    assert "Initial Residual = %E" % np.sqrt(w["rr"][0]) in txt
    shown = 0
    for j in range(1, w["k"]):
        if j % freq == 0 or j + 1 == itermax:
            assert "Iteration = %d Residual = %E" % (j, np.sqrt(w["rr"][j - 1])) in txt, j
            shown += 1
    assert shown >= 1 and len(re.findall(r"^Iteration = ", txt, re.M)) == shown
    assert re.search(r"^Solution performed %d iterations and took \d+\.\d\ds$" % w["k"], txt, re.M)


@pytest.mark.parametrize("exe", ["sparseBench-CRS-HIP", "sparseBench-SCS-HIP"])
def test_driver_runs_bicgstab(gpu, exe, wants):
    for key, args in (("cd", ["-m", wants["path"]]), ("hpcg", ["-x", "16", "-y", "16", "-z", "16"])):
        out = run([os.path.join(BIN, exe), "-t", "bicgstab", "-i", str(ITERMAX), "-e", repr(EPS)] + args)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        txt = out.stdout.decode()
        assert "Test type: BiCGStab" in txt
        check_lines(txt, wants[key], ITERMAX)
        assert ("Difference between computed and exact  = " in txt) == (key == "hpcg")
        assert "Function   Rate(MB/s)  Rate(MFlop/s)  Walltime(s)" in txt


def test_driver_help_and_refusals(gpu):
    crs = os.path.join(BIN, "sparseBench-CRS-HIP")
    help_text = run([crs, "-h"]).stdout.decode()
    assert re.search(r"-t <bench type>.*\bbicgstab\b", help_text, re.S) and re.search(r"-t <bench type>.*\bpcg\b", help_text)
    size = ["-x", "8", "-y", "8", "-z", "8", "-i", "10"]
    for exe in ("sparseBench-CRS-HIP-SP", "sparseBench-SCS-HIP-SP"):
        out = run([os.path.join(BIN, exe), "-t", "bicgstab"] + size)
        assert out.returncode == 1 and "BiCGStab: double precision only" in out.stderr.decode()
    out = run([crs, "-t", "cheb"] + size)
    assert out.returncode == 1 and "Unknown solver type cheb" in out.stdout.decode()
    out = run([crs, "-t", "bicgstab", "-n", "2"] + size)
    assert out.returncode == 1 and "-t cg only" in out.stderr.decode()


def build(fmt, tmp_path, sp):
    exe = os.path.join(str(tmp_path), "bicgstab_driver_%s%s" % (fmt, "_sp" if sp else ""))
    suffix = "_sp" if sp else ""
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-Wall"] + (["-DPRECISION=1"] if sp else []) +
                          ["-D" + fmt, "-I" + os.path.join(ROOT, "include"), "-DSOLVER_BICGSTAB", os.path.join(ROOT, "tests", "c", "solver_driver.c"), "-o", exe,
                           "-L" + LIB, "-lsparsebench_%s%s" % (fmt.lower(), suffix), "-lsparsebench_host%s" % suffix, "-lsbhip",
                           "-Wl,-rpath," + LIB, "-lm"])
    return exe


@pytest.mark.parametrize("fmt", ["CRS", "SCS"])
def test_c_caller_of_solveBiCGStab(gpu, fmt, wants, tmp_path):
    exe = build(fmt, tmp_path, sp=False)
    for key, arg in (("cd", wants["path"]), ("hpcg", "16")):
        out = run([exe, arg, str(ITERMAX), repr(EPS)])
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        txt = out.stdout.decode()
        assert int(re.search(r"^k (\d+)$", txt, re.M).group(1)) == wants[key]["k"]
        check_lines(txt, wants[key], ITERMAX)


@pytest.mark.parametrize("fmt", ["CRS", "SCS"])
def test_sp_library_refuses_solveBiCGStab(gpu, fmt, tmp_path):
    exe = build(fmt, tmp_path, sp=True)
    out = run([exe, "8", "10", "0.0"])
    assert out.returncode == 1 and "BiCGStab: double precision only" in out.stderr.decode()
