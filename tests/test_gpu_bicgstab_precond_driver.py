"""`-t bicgstab -P <precond>` from the benchmark drivers and solveBiCGStabPrecond from both drop-in libraries (a C caller written
against include/sparsebench/sparsebench.h only), against the CPU restatement of BiCGStab under a preconditioner plan
(tests/bicgstab_precond_ref.py): `-P poly -d 3` on convection-diffusion 16^3 from a Matrix Market file and on the generated 16^3
stencil prints the k of tests/golden/bicgstab_precond_hist.json's CRS case and the restatement's residuals; and the switch's
refusals."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import bicgstab_precond_cases as cases
import bicgstab_precond_ref as pref
import bicgstab_ref as ref
from test_gpu_bicgstab_driver import check_lines, run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")
BIN = os.path.join(ROOT, "sparsebench_amd", "bin")
ITERMAX = 40  # the lines are printed every itermax / 10 iterations: some fall before the k of both matrices (18 and 10)


@pytest.fixture(scope="module")
def wants(tmp_path_factory):
    """restatement runs in the drivers' formats: CRS and Sell-64-1 (the same order: sigma = 1), poly (3, 16), eps = 1e-10 ||b||"""
    tmp = tmp_path_factory.mktemp("bicgstab_precond_driver")
    out = {"path": ref.matrix_path(("cd", 16, 16, 16), tmp)}
    for key, matrix in (("cd", ("cd", 16, 16, 16)), ("hpcg", ("hpcg", 16))):
        out[key] = pref.run_case(dict(cases.CASES["cd16_crs_poly_3_16"], matrix=matrix, itermax=ITERMAX), tmp)
        assert 1 < out[key]["k"] < ITERMAX
    with open(os.path.join(ROOT, "tests", "golden", "bicgstab_precond_hist.json")) as f:
        assert out["cd"]["k"] == json.load(f)["cases"]["cd16_crs_poly_3_16"]["k"]
    return out


@pytest.mark.parametrize("exe", ["sparseBench-CRS-HIP", "sparseBench-SCS-HIP"])
def test_driver_runs_bicgstab_with_the_polynomial(gpu, exe, wants):
    for key, args in (("cd", ["-m", wants["path"]]), ("hpcg", ["-x", "16", "-y", "16", "-z", "16"])):
        w = wants[key]
        out = run([os.path.join(BIN, exe), "-t", "bicgstab", "-P", "poly", "-d", "3", "-i", str(ITERMAX), "-e", repr(float(w["eps"]))] + args)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        txt = out.stdout.decode()
        assert "Test type: BiCGStab" in txt
        assert re.search(r"^Preconditioner: Chebyshev polynomial, steps = 3, lambda in \[", txt, re.M)
        check_lines(txt, w, ITERMAX)
        assert ("Difference between computed and exact  = " in txt) == (key == "hpcg")


def test_driver_runs_the_other_plans(gpu):
    """each prints PCG's own preconditioner line and converges on the generated 16^3"""
    scs = os.path.join(BIN, "sparseBench-SCS-HIP")
    size = ["-x", "16", "-y", "16", "-z", "16", "-i", "60", "-e", "1e-6"]
    for args, line in ((["-P", "sgs"], r"Preconditioner: SGS \(multicolour symmetric Gauss-Seidel\), nC = \d+"),
                       (["-P", "mgpoly", "-g", "-d", "1"], r"Preconditioner: MG \(V-cycle, full-weighting transfers, Chebyshev polynomial "
                                                         r"smoother, Galerkin coarse operators\), levels = 4, steps = 1"),
                       (["-P", "mgfw", "-l", "2"], r"Preconditioner: MG \(V-cycle, full-weighting transfers, multicolour SGS smoother\), levels = 2")):
        out = run([scs, "-t", "bicgstab"] + args + size)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        txt = out.stdout.decode()
        assert re.search(line, txt), txt[-1500:]
        k = int(re.search(r"^Solution performed (\d+) iterations", txt, re.M).group(1))
        assert 1 < k < 60, (args, k)


def test_switch_refusals(gpu):
    crs = os.path.join(BIN, "sparseBench-CRS-HIP")
    help_text = run([crs, "-h"]).stdout.decode()
    assert re.search(r"^  -P <sgs\|mg\|mgfw\|poly\|mgpoly>.*-t bicgstab", help_text, re.M)
    assert re.search(r"-p <jacobi\|sgs>.*Default jacobi", help_text) and "-C <int>" in help_text and "-g " in help_text  # still whole
    size = ["-x", "8", "-y", "8", "-z", "8", "-i", "10"]
    for args, msg in ((["-t", "bicgstab", "-p", "sgs"], "goes with -t pcg only"),
                      (["-t", "pcg", "-P", "sgs"], "goes with -t bicgstab only"),
                      (["-P", "poly"], "goes with -t bicgstab only"),
                      (["-t", "bicgstab", "-P", "jacobi"], "Unknown preconditioner jacobi (-P <sgs|mg|mgfw|poly|mgpoly>)"),
                      (["-t", "bicgstab", "-P", "sgs", "-d", "3"], "-d <int> (the steps) goes with -p poly only"),
                      (["-t", "bicgstab", "-P", "poly", "-l", "2"], "-l <int> (the levels) goes with -p mg only"),
                      (["-t", "bicgstab", "-P", "poly", "-g"], "-g (Galerkin coarse operators) goes with -p mgpoly only"),
                      (["-t", "bicgstab", "-l", "2"], "-l <int> (the levels) goes with -p mg only"),
                      (["-t", "bicgstab", "-P", "mg", "-l", "5"], "levels"),
                      (["-t", "bicgstab", "-P", "mgpoly", "-m", "some.mtx"], "-P mgpoly needs the grid")):
        out = run([crs] + args + size)
        assert out.returncode == 1 and msg in out.stderr.decode(), (args, out.returncode, out.stderr.decode()[-500:])
    for exe in ("sparseBench-CRS-HIP-SP", "sparseBench-SCS-HIP-SP"):
        out = run([os.path.join(BIN, exe), "-t", "bicgstab", "-P", "poly"] + size)
        assert out.returncode == 1 and "BiCGStab: double precision only" in out.stderr.decode()


def build(fmt, tmp_path, sp):
    exe = os.path.join(str(tmp_path), "bicgstab_precond_driver_%s%s" % (fmt, "_sp" if sp else ""))
    suffix = "_sp" if sp else ""
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-Wall"] + (["-DPRECISION=1"] if sp else []) +
                          ["-D" + fmt, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "bicgstab_precond_driver.c"), "-o", exe,
                           "-L" + LIB, "-lsparsebench_%s%s" % (fmt.lower(), suffix), "-lsparsebench_host%s" % suffix, "-lsbhip",
                           "-Wl,-rpath," + LIB, "-lm"])
    return exe


@pytest.mark.parametrize("fmt", ["CRS", "SCS"])
def test_c_caller_of_solveBiCGStabPrecond(gpu, fmt, wants, tmp_path):
    exe = build(fmt, tmp_path, sp=False)
    for key, arg in (("cd", wants["path"]), ("hpcg", "16")):
        w = wants[key]
        out = run([exe, arg, str(ITERMAX), repr(float(w["eps"])), "4"])  # poly at its default 3 steps
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        txt = out.stdout.decode()
        assert int(re.search(r"^k (\d+)$", txt, re.M).group(1)) == w["k"]
        assert "Preconditioner: Chebyshev polynomial, steps = 3" in txt
        check_lines(txt, w, ITERMAX)
    out = run([exe, wants["path"], "10", "0.0", "2"])  # a V-cycle on a file matrix
    assert out.returncode == 1 and "MG: needs the grid" in out.stderr.decode()


@pytest.mark.parametrize("fmt", ["CRS", "SCS"])
def test_sp_library_refuses_solveBiCGStabPrecond(gpu, fmt, tmp_path):
    exe = build(fmt, tmp_path, sp=True)
    out = run([exe, "8", "10", "0.0", "4"])
    assert out.returncode == 1 and "BiCGStab: double precision only" in out.stderr.decode()
