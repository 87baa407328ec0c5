"""`-t gmres` from the benchmark drivers and solveGMRES from both drop-in libraries (a C caller written against
include/sparsebench/sparsebench.h only), against the iteration count of the CPU restatement."""
import os
import re
import subprocess

import pytest

import gmres_cases
import gmres_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")
BIN = os.path.join(ROOT, "sparsebench_amd", "bin")


@pytest.fixture(scope="module")
def cd16(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gmres_driver")
    want = gmres_ref.run_case("cd16_m30", tmp)
    return os.path.join(str(tmp), "cd_16_16_16.mtx"), want


def run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


@pytest.mark.parametrize("exe", ["sparseBench-CRS-HIP", "sparseBench-SCS-HIP"])
def test_driver_runs_gmres(gpu, exe, cd16):
    mtx, want = cd16
    out = run([os.path.join(BIN, exe), "-t", "gmres", "-m", mtx, "-i", "150", "-e", repr(want["eps"]), "-r", "30"])
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    txt = out.stdout.decode()
    assert "Test type: GMRES" in txt
    assert "Initial Residual = %E" % want["res"][0] in txt
    for j in (15, 30, 45, 60, 75, 90, 105):
        assert "Iteration = %d Residual = %E" % (j, want["res"][j]) in txt, j
    assert re.search(r"Solution performed %d iterations and took \d+\.\d\ds" % want["k"], txt)
    assert "Function   Rate(MB/s)  Rate(MFlop/s)  Walltime(s)" in txt
    # another restart length is another solve
    w10 = gmres_ref.run_case("cd16_m10", os.path.dirname(mtx))
    out = run([os.path.join(BIN, exe), "-t", "gmres", "-m", mtx, "-i", "150", "-e", repr(want["eps"]), "-r", "10"])
    assert re.search(r"Solution performed %d iterations" % w10["k"], out.stdout.decode())


def test_driver_unknown_type_and_sp_refusal(gpu, cd16):
    mtx, _ = cd16
    for t in ("nonsense", "cheb"):
        out = run([os.path.join(BIN, "sparseBench-CRS-HIP"), "-t", t])
        assert out.returncode == 1 and "Unknown solver type %s" % t in out.stdout.decode()
    for exe in ("sparseBench-CRS-HIP-SP", "sparseBench-SCS-HIP-SP"):
        out = run([os.path.join(BIN, exe), "-t", "gmres", "-m", mtx])
        assert out.returncode == 1 and "GMRES: double precision only" in out.stderr.decode()
    assert "gmres" in run([os.path.join(BIN, "sparseBench-CRS-HIP"), "-h"]).stdout.decode()


@pytest.mark.parametrize("fmt", ["CRS", "SCS"])
def test_c_caller_of_solveGMRES(gpu, fmt, cd16, tmp_path):
    mtx, want = cd16
    exe = os.path.join(str(tmp_path), "gmres_driver_%s" % fmt)
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-Wall", "-D" + fmt, "-I" + os.path.join(ROOT, "include"),
                           "-DSOLVER_GMRES", os.path.join(ROOT, "tests", "c", "solver_driver.c"), "-o", exe, "-L" + LIB,
                           "-lsparsebench_%s" % fmt.lower(), "-lsparsebench_host", "-lsbhip", "-Wl,-rpath," + LIB, "-lm"])
    out = run([exe, mtx, "150", repr(want["eps"]), "30"])
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    txt = out.stdout.decode()
    assert int(re.search(r"^k (\d+)$", txt, re.M).group(1)) == want["k"]
    assert "Initial Residual = %E" % want["res"][0] in txt
