"""`-t pcg -p mg` from the benchmark drivers and solvePCGMG through a drop-in library: the preconditioner line and
the iteration count of tests/golden/mg_hist.json at 16^3; the switches' refusals."""
import math
import os
import re
import subprocess

import pytest

import mg_cases
from conftest import load_json

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sparsebench_amd", "bin")
SIZE = ["-x", "16", "-y", "16", "-z", "16"]


def run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def case_args(e, c):
    """the golden case's itermax and eps on the command line (%.17g reads back to the same double)"""
    return ["-i", str(c["itermax"]), "-e", "%.17g" % float.fromhex(e["eps"])]


@pytest.mark.parametrize("exe", ["sparseBench-CRS-HIP", "sparseBench-SCS-HIP"])
def test_driver_runs_mg_pcg(gpu, exe):
    """CRS and Sell-64-1 (the driver's default) walk the natural order: the golden's CRS cases"""
    golden = load_json("mg_hist.json")["cases"]
    for levels, name in ((["-l", "3"], "hpcg16_crs_L3"), ([], "hpcg16_crs_L4")):  # without -l: auto, HPCG's depth at 16^3
        e, c = golden[name], mg_cases.CASES[name]
        out = run([os.path.join(BIN, exe), "-t", "pcg", "-p", "mg"] + levels + case_args(e, c) + SIZE)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        txt = out.stdout.decode()
        assert re.search(r"^Test type: PCG\n(Generate .*\n)*Preconditioner: MG \(V-cycle, multicolour SGS smoother\), levels = %d, nC = %d$"
                         % (e["L"], e["nC"][0]), txt, re.M), txt[-2000:]
        assert 1 < e["k"] < c["itermax"]
        assert re.search(r"^Solution performed %d iterations and took \d+\.\d\ds$" % e["k"], txt, re.M), txt[-2000:]
        assert "Difference between computed and exact  = 0.0000" in txt


def test_driver_in_a_permuted_order_shows_the_hierarchy_it_built(gpu):
    """CRS and Sell-64-1 walk the natural order, where no bit of the output depends on the coarse levels
    (test_mg_host.py::test_in_the_natural_order_the_coarse_levels_are_idle).  With -s 256 it does: the residual lines of -l 3 and of
    the auto depth (solvePCGMG's own hierarchy, four levels) are the golden file's, and they differ from each other"""
    golden = load_json("mg_hist.json")["cases"]
    exe = os.path.join(BIN, "sparseBench-SCS-HIP")
    printed = {}
    for levels, name in ((["-l", "3"], "hpcg16_sell_64_256_L3_i20"), ([], "hpcg16_sell_64_256_L4_i20")):
        e, c = golden[name], mg_cases.CASES[name]
        rr = [float.fromhex(v) for v in e["rr"]]
        assert c["itermax"] == e["k"] == 20 and (c["C"], c["sigma"]) == (64, 256)
        out = run([exe, "-t", "pcg", "-p", "mg", "-C", "64", "-s", "256"] + levels + case_args(e, c) + SIZE)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        txt = out.stdout.decode()
        assert "levels = %d, nC = %d" % (e["L"], e["nC"][0]) in txt
        lines = ["Initial Residual = %E" % math.sqrt(rr[0])] + ["Iteration = %d Residual = %E" % (j, math.sqrt(rr[j - 1])) for j in range(2, 20, 2)]
        lines.append("Iteration = 19 Residual = %E" % math.sqrt(rr[18]))
        for line in lines:
            assert line in txt, (name, line, txt[-2000:])
        assert re.search(r"^Solution performed 20 iterations", txt, re.M)
        printed[name] = lines
    differing = [a for a, b in zip(*printed.values()) if a != b]
    assert len(differing) >= 8, differing  # the depth shows in nearly every printed line


def test_solvePCGMG_through_the_dropin_library(gpu, tmp_path):
    """the drop-in entry at auto depth, run by a C caller of its own, gives what the driver without -l gives: the same k and
    lines, through the SCS library with the Sell-64-1 default and through the CRS one -- and the symbol is the library's own"""
    import ctypes
    import driver_options
    from sparsebench_amd import hostapi
    hostapi.host()
    golden = load_json("mg_hist.json")["cases"]
    e, c = golden["hpcg16_crs_L4"], mg_cases.CASES["hpcg16_crs_L4"]
    rr = [float.fromhex(v) for v in e["rr"]]
    for fmt, exe in (("crs", "sparseBench-CRS-HIP"), ("scs", "sparseBench-SCS-HIP")):
        d = ctypes.CDLL(os.path.join(ROOT, "sparsebench_amd", "lib", "libsparsebench_%s.so" % fmt))
        assert hasattr(d, "solvePCGMG")
        ldd = run(["ldd", os.path.join(BIN, exe)]).stdout.decode()
        assert "libsparsebench_%s.so" % fmt in ldd
        called, k = driver_options.run_dropin_symbol(tmp_path, fmt.upper(), "SOLVER_PCG_MG", ["16"] + case_args(e, c)[1::2])
        assert k == e["k"]
        txt = run([os.path.join(BIN, exe), "-t", "pcg", "-p", "mg"] + case_args(e, c) + SIZE).stdout.decode()
        for out in (called, txt):
            assert re.search(r"^Preconditioner: MG \(V-cycle, multicolour SGS smoother\), levels = 4, nC = %d$" % e["nC"][0], out, re.M), out[-2000:]
            assert "Initial Residual = %E" % math.sqrt(rr[0]) in out and "Iteration = 15 Residual = %E" % math.sqrt(rr[14]) in out
            assert re.search(r"^Solution performed %d iterations" % e["k"], out, re.M), out[-2000:]


def test_switch_refusals(gpu, tmp_path):
    crs = os.path.join(BIN, "sparseBench-CRS-HIP")
    small = ["-i", "10"]
    help_text = run([crs, "-h"]).stdout.decode()
    assert re.search(r"-p mg\b", help_text) and "-l <int>" in help_text and re.search(r"-p <jacobi\|sgs>", help_text)
    mtx = tmp_path / "tri.mtx"
    mg_cases.tridiagonal(str(mtx), 20, 4.0)
    out = run([crs, "-t", "pcg", "-p", "mg", "-m", str(mtx)] + small)
    assert out.returncode == 1 and "needs the grid" in out.stderr.decode(), out.stderr.decode()
    for extra in ([], ["-p", "sgs"], ["-p", "jacobi"]):
        out = run([crs, "-t", "pcg", "-l", "2"] + extra + small + SIZE)
        assert out.returncode == 1 and "goes with -p mg only" in out.stderr.decode(), extra
    out = run([crs, "-t", "pcg", "-p", "mg", "-l", "5"] + small + SIZE)
    assert out.returncode == 1 and "5 levels would give a coarse dimension smaller than 2" in out.stderr.decode()
    out = run([crs, "-t", "pcg", "-p", "mg", "-l", "2", "-x", "15", "-y", "16", "-z", "16"] + small)
    assert out.returncode == 1 and "2 levels need every dimension divisible by 2" in out.stderr.decode()
    out = run([crs, "-t", "cg", "-p", "mg"] + small + SIZE)
    assert out.returncode == 1 and "goes with -t pcg only" in out.stderr.decode()
    for exe in ("sparseBench-CRS-HIP-SP", "sparseBench-SCS-HIP-SP"):
        out = run([os.path.join(BIN, exe), "-t", "pcg", "-p", "mg"] + small + SIZE)
        assert out.returncode == 1 and "PCG: double precision only" in out.stderr.decode()
