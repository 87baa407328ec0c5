"""`-t gmres -r <m> -P <precond>` from the benchmark drivers and solveGMRESPrecond from both drop-in libraries (a C caller written
against include/sparsebench/sparsebench.h only), against the CPU restatement of right-preconditioned GMRES
(tests/gmres_precond_ref.py): `-r 10 -P poly -d 3` on convection-diffusion 16^3 from a Matrix Market file and on the generated 16^3
stencil prints the k of tests/golden/gmres_precond_hist.json's table and the restatement's residual estimates; the preconditioner
lines; and the switch's refusals."""
import json
import os
import re
import subprocess

import pytest

import bicgstab_ref
import gmres_precond_cases as cases
import gmres_precond_ref as ref
from test_gpu_gmres_driver import run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")
BIN = os.path.join(ROOT, "sparsebench_amd", "bin")
ITERMAX = 100  # the lines are printed every itermax / 10 iterations: some fall before the k of both matrices (44 and 16)
M = 10


@pytest.fixture(scope="module")
def wants(tmp_path_factory):
    """restatement runs in the drivers' formats: CRS and Sell-64-1 (the same order: sigma = 1), poly (3, 16), eps = 1e-10 ||b||"""
    tmp = tmp_path_factory.mktemp("gmres_precond_driver")
    out = {"path": bicgstab_ref.matrix_path(cases.CD16, tmp)}
    with open(os.path.join(ROOT, "tests", "golden", "gmres_precond_hist.json")) as f:
        table = json.load(f)["table"]
    for key, matrix in (("cd", cases.CD16), ("hpcg", cases.HPCG16)):
        out[key] = ref.run_case(dict(cases.table_case(matrix, M, "poly"), itermax=ITERMAX), tmp)
        assert 10 < out[key]["k"] == table["%s m%d poly" % ("_".join(str(v) for v in matrix), M)] < ITERMAX
    return out


def check_lines(txt, w):
    assert "Initial Residual = %E" % w["res"][0] in txt
    shown = [j for j in range(ITERMAX // 10, w["k"], ITERMAX // 10)]
    assert shown
    for j in shown:
        assert "Iteration = %d Residual = %E" % (j, w["res"][j]) in txt, j
    assert re.search(r"Solution performed %d iterations and took \d+\.\d\ds" % w["k"], txt)


@pytest.mark.parametrize("exe", ["sparseBench-CRS-HIP", "sparseBench-SCS-HIP"])
def test_driver_runs_gmres_with_the_polynomial(gpu, exe, wants):
    for key, args in (("cd", ["-m", wants["path"]]), ("hpcg", ["-x", "16", "-y", "16", "-z", "16"])):
        w = wants[key]
        out = run([os.path.join(BIN, exe), "-t", "gmres", "-r", str(M), "-P", "poly", "-d", "3", "-i", str(ITERMAX), "-e", repr(float(w["eps"]))] + args)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        txt = out.stdout.decode()
        assert "Test type: GMRES" in txt
        assert re.search(r"^Preconditioner: Chebyshev polynomial, steps = 3, lambda in \[", txt, re.M)
        check_lines(txt, w)
        assert ("Difference between computed and exact  = " in txt) == (key == "hpcg")


def test_driver_prints_the_preconditioner_lines(gpu):
    """each prints PCG's own preconditioner line and converges on the generated 16^3"""
    scs = os.path.join(BIN, "sparseBench-SCS-HIP")
    size = ["-x", "16", "-y", "16", "-z", "16", "-i", "60", "-e", "1e-6", "-r", "10"]
    for args, line in ((["-P", "sgs"], r"Preconditioner: SGS \(multicolour symmetric Gauss-Seidel\), nC = \d+"),
                       (["-P", "mgpoly", "-g", "-d", "1"], r"Preconditioner: MG \(V-cycle, full-weighting transfers, Chebyshev polynomial "
                                                         r"smoother, Galerkin coarse operators\), levels = 4, steps = 1"),
                       (["-P", "jacobi"], r"Preconditioner: Jacobi \(diagonal\), nC = 0")):
        out = run([scs, "-t", "gmres"] + args + size)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        txt = out.stdout.decode()
        assert re.search(line, txt), txt[-1500:]
        k = int(re.search(r"^Solution performed (\d+) iterations", txt, re.M).group(1))
        assert 1 < k < 60, (args, k)
    out = run([scs, "-t", "gmres"] + size)  # without -P: no preconditioner line
    assert out.returncode == 0 and "Preconditioner:" not in out.stdout.decode()


def test_switch_refusals(gpu):
    crs = os.path.join(BIN, "sparseBench-CRS-HIP")
    help_text = run([crs, "-h"]).stdout.decode()
    assert re.search(r"^  -P <sgs\|mg\|mgfw\|poly\|mgpoly>.*-t bicgstab", help_text, re.M) and re.search(r"-t gmres.*-P jacobi", help_text)
    assert re.search(r"-p <jacobi\|sgs>.*Default jacobi", help_text) and "-C <int>" in help_text and "-r <int>" in help_text  # still whole
    size = ["-x", "8", "-y", "8", "-z", "8", "-i", "10"]
    for args, msg in ((["-t", "gmres", "-p", "sgs"], "goes with -t pcg only"),
                      (["-t", "pcg", "-P", "sgs"], "goes with -t bicgstab only"),
                      (["-P", "poly"], "goes with -t bicgstab only"),
                      (["-t", "pcg", "-P", "jacobi"], "Unknown preconditioner jacobi (-P <sgs|mg|mgfw|poly|mgpoly>)"),
                      (["-t", "bicgstab", "-P", "jacobi"], "Unknown preconditioner jacobi (-P <sgs|mg|mgfw|poly|mgpoly>)"),
                      (["-t", "gmres", "-P", "ilu"], "Unknown preconditioner ilu"),
                      (["-t", "gmres", "-P", "sgs", "-d", "3"], "-d <int> (the steps) goes with -p poly only"),
                      (["-t", "gmres", "-P", "jacobi", "-l", "2"], "-l <int> (the levels) goes with -p mg only"),
                      (["-t", "gmres", "-P", "poly", "-g"], "-g (Galerkin coarse operators) goes with -p mgpoly only"),
                      (["-t", "gmres", "-l", "2"], "-l <int> (the levels) goes with -p mg only"),
                      (["-t", "gmres", "-P", "mgpoly", "-a", "-g"], "it does not go with -g"),
                      (["-t", "gmres", "-P", "mgpoly", "-m", "some.mtx"], "-P mgpoly needs the grid")):
        out = run([crs] + args + size)
        assert out.returncode == 1 and msg in out.stderr.decode(), (args, out.returncode, out.stderr.decode()[-500:])
        assert "Setup took" not in out.stdout.decode()
    for exe in ("sparseBench-CRS-HIP-SP", "sparseBench-SCS-HIP-SP"):
        out = run([os.path.join(BIN, exe), "-t", "gmres", "-P", "poly"] + size)
        assert out.returncode == 1 and "GMRES: double precision only" in out.stderr.decode()


def build(fmt, tmp_path, sp):
    exe = os.path.join(str(tmp_path), "gmres_precond_driver_%s%s" % (fmt, "_sp" if sp else ""))
    suffix = "_sp" if sp else ""
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-Wall"] + (["-DPRECISION=1"] if sp else []) +
                          ["-D" + fmt, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "gmres_precond_driver.c"), "-o", exe,
                           "-L" + LIB, "-lsparsebench_%s%s" % (fmt.lower(), suffix), "-lsparsebench_host%s" % suffix, "-lsbhip",
                           "-Wl,-rpath," + LIB, "-lm"])
    return exe


@pytest.mark.parametrize("fmt", ["CRS", "SCS"])
def test_c_caller_of_solveGMRESPrecond(gpu, fmt, wants, tmp_path):
    exe = build(fmt, tmp_path, sp=False)
    for key, arg in (("cd", wants["path"]), ("hpcg", "16")):
        w = wants[key]
        out = run([exe, arg, str(ITERMAX), repr(float(w["eps"])), str(M), "4"])  # poly at its default 3 steps
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        txt = out.stdout.decode()
        assert int(re.search(r"^k (\d+)$", txt, re.M).group(1)) == w["k"]
        assert "Preconditioner: Chebyshev polynomial, steps = 3" in txt
        check_lines(txt, w)
    out = run([exe, "16", "60", "1e-6", str(M), "0"])
    assert out.returncode == 0 and "Preconditioner: Jacobi (diagonal), nC = 0" in out.stdout.decode()
    out = run([exe, wants["path"], "10", "0.0", str(M), "2"])  # a V-cycle on a file matrix
    assert out.returncode == 1 and "MG: needs the grid" in out.stderr.decode()
    out = run([exe, "8", "10", "0.0", str(M), "6"])
    assert out.returncode == 1 and "GMRES: the preconditioners are 0 jacobi" in out.stderr.decode()


@pytest.mark.parametrize("fmt", ["CRS", "SCS"])
def test_sp_library_refuses_solveGMRESPrecond(gpu, fmt, tmp_path):
    exe = build(fmt, tmp_path, sp=True)
    out = run([exe, "8", "10", "0.0", "10", "4"])
    assert out.returncode == 1 and "GMRES: double precision only" in out.stderr.decode()
