"""`-t pcg -p mgpoly` from the benchmark drivers and solvePCGMGPoly through a drop-in library: the preconditioner
line, the iteration count and every printed residual of tests/golden/mg_poly_hist.json at 16^3, in the natural order (CRS) and in
a permuted one (-s 256), at -l 3 -d 2 and at the defaults; `-p mgfw` and `-p poly` print what they printed; the switches'
refusals."""
import ctypes
import math
import os
import re
import subprocess

import pytest

import mg_cases
import mg_poly_cases as cases
from conftest import load_json

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sparsebench_amd", "bin")
SIZE = ["-x", "16", "-y", "16", "-z", "16"]
LINE = (r"Preconditioner: MG \(V-cycle, full-weighting transfers, Chebyshev polynomial smoother\), levels = %d, steps = %d, "
        r"lambda in \[%s, %s\]")


def run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def check_output(txt, e, steps, head=r"^Test type: PCG\n(Generate .*\n)*"):
    """the golden case's k, and with -i 19 (a line per iteration) the residual every iteration starts from, the last included;
    head: what stands before the preconditioner's line (the driver's own lines; "^" for a caller that prints none)"""
    rr = [float.fromhex(v) for v in e["rr"]]
    assert 1 < e["k"] < 19 and len(rr) == e["k"] - 1
    iv = tuple(re.escape("%.6g" % float.fromhex(v)) for v in e["intervals"][0])
    assert re.search(head + LINE % ((e["L"], steps) + iv) + "$", txt, re.M), txt[-2000:]
    lines = ["Initial Residual = %E" % math.sqrt(rr[0])] + ["Iteration = %d Residual = %E" % (j, math.sqrt(rr[j - 1])) for j in range(1, e["k"])]
    for line in lines:
        assert line in txt, (line, txt[-2000:])
    assert "Iteration = %d Residual" % e["k"] not in txt
    assert re.search(r"^Solution performed %d iterations and took \d+\.\d\ds$" % e["k"], txt, re.M), txt[-2000:]
    assert "Difference between computed and exact  = 0.0000" in txt
    return lines


@pytest.mark.parametrize("exe,order,names", [
    ("sparseBench-CRS-HIP", [], ("hpcg16_crs_L3", "hpcg16_crs_L4")),
    ("sparseBench-SCS-HIP", ["-C", "64", "-s", "256"], ("hpcg16_sell_64_256_L3", "hpcg16_sell_64_256_L4"))])
def test_driver_runs_mgpoly_pcg(gpu, exe, order, names):
    golden = load_json("mg_poly_hist.json")["cases"]
    printed = []
    for switches, name in zip((["-l", "3", "-d", "2"], []), names):  # without -l and -d: HPCG's depth, 2 steps, through solvePCGMGPoly
        e, c = golden[name], cases.CASES[name]
        assert (c["C"], c["sigma"]) == ((64, 256) if order else (64, 1)) and c.get("steps") is None and not c.get("galerkin")
        out = run([os.path.join(BIN, exe), "-t", "pcg", "-p", "mgpoly"] + order + switches + ["-i", "19", "-e", "%.17g" % float.fromhex(e["eps"])] + SIZE)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        printed.append(check_output(out.stdout.decode(), e, 2))
    assert [a for a, b in zip(*printed) if a != b]  # the depth shows in the printed residuals


def test_driver_takes_another_step_count(gpu):
    e = load_json("mg_poly_hist.json")["cases"]["hpcg16_sell_64_256_L3_steps1"]
    out = run([os.path.join(BIN, "sparseBench-SCS-HIP"), "-t", "pcg", "-p", "mgpoly", "-C", "64", "-s", "256", "-l", "3", "-d", "1", "-i", "19",
               "-e", "%.17g" % float.fromhex(e["eps"])] + SIZE)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    check_output(out.stdout.decode(), e, 1)


def test_solvePCGMGPoly_through_the_dropin_library(gpu, tmp_path):
    """the symbol, run by a C caller of its own, and the driver at the defaults: both the golden case's lines"""
    import driver_options
    from sparsebench_amd import hostapi
    hostapi.host()
    e = load_json("mg_poly_hist.json")["cases"]["hpcg16_crs_L4"]
    for fmt, exe in (("crs", "sparseBench-CRS-HIP"), ("scs", "sparseBench-SCS-HIP")):  # (Sell-64-1, the default: the natural order)
        d = ctypes.CDLL(os.path.join(ROOT, "sparsebench_amd", "lib", "libsparsebench_%s.so" % fmt))
        assert hasattr(d, "solvePCGMGPoly")
        assert "libsparsebench_%s.so" % fmt in run(["ldd", os.path.join(BIN, exe)]).stdout.decode()
        called, k = driver_options.run_dropin_symbol(tmp_path, fmt.upper(), "SOLVER_PCG_MGPOLY", ["16", "19", "%.17g" % float.fromhex(e["eps"])])
        assert k == e["k"]
        check_output(called, e, 2, head="^")
        txt = run([os.path.join(BIN, exe), "-t", "pcg", "-p", "mgpoly", "-i", "19", "-e", "%.17g" % float.fromhex(e["eps"])] + SIZE).stdout.decode()
        check_output(txt, e, 2)


def test_mgfw_and_poly_output_is_unchanged(gpu):
    crs = os.path.join(BIN, "sparseBench-CRS-HIP")
    e = load_json("mg_fw_hist.json")["cases"]["hpcg16_crs_L3"]
    out = run([crs, "-t", "pcg", "-p", "mgfw", "-l", "3", "-i", "19", "-e", "%.17g" % float.fromhex(e["eps"])] + SIZE)
    txt = out.stdout.decode()
    assert out.returncode == 0 and "Chebyshev" not in txt
    assert re.search(r"^Preconditioner: MG \(V-cycle, full-weighting transfers, multicolour SGS smoother\), levels = 3, nC = %d$" % e["nC"][0],
                     txt, re.M), txt[-2000:]
    assert re.search(r"^Solution performed %d iterations" % e["k"], txt, re.M)
    out = run([crs, "-t", "pcg", "-p", "poly", "-d", "2", "-i", "30"] + SIZE)
    txt = out.stdout.decode()
    assert out.returncode == 0 and re.search(r"^Preconditioner: Chebyshev polynomial, steps = 2, lambda in \[", txt, re.M) and "V-cycle" not in txt


def test_switch_refusals(gpu, tmp_path):
    crs = os.path.join(BIN, "sparseBench-CRS-HIP")
    small = ["-i", "10"]
    help_text = run([crs, "-h"]).stdout.decode()
    assert re.search(r"-p mgpoly\b", help_text) and re.search(r"-p mgfw\b", help_text) and re.search(r"-p poly\b", help_text)
    mtx = tmp_path / "tri.mtx"
    mg_cases.tridiagonal(str(mtx), 20, 4.0)
    out = run([crs, "-t", "pcg", "-p", "mgpoly", "-m", str(mtx)] + small)
    assert out.returncode == 1 and "-p mgpoly needs the grid" in out.stderr.decode(), out.stderr.decode()
    out = run([crs, "-t", "pcg", "-p", "mgpoly", "-l", "5"] + small + SIZE)
    assert out.returncode == 1 and "5 levels would give a coarse dimension smaller than 2" in out.stderr.decode()
    out = run([crs, "-t", "pcg", "-p", "mgpoly", "-l", "2", "-x", "15", "-y", "16", "-z", "16"] + small)
    assert out.returncode == 1 and "2 levels need every dimension divisible by 2" in out.stderr.decode()
    for bad in ("0", "17", "x"):
        out = run([crs, "-t", "pcg", "-p", "mgpoly", "-d", bad] + small + SIZE)
        assert out.returncode == 1 and "-d <int> (the steps of -p poly or -p mgpoly) must be 1 to 16" in out.stderr.decode(), bad
    out = run([crs, "-t", "pcg", "-p", "mgfw", "-d", "2"] + small + SIZE)
    assert out.returncode == 1 and "-d <int> (the steps) goes with -p poly only, or with -p mgpoly" in out.stderr.decode()
    out = run([crs, "-t", "pcg", "-p", "sgs", "-l", "2"] + small + SIZE)
    assert out.returncode == 1 and "-l <int> (the levels) goes with -p mg only, or with -p mgfw or -p mgpoly" in out.stderr.decode()
    out = run([crs, "-t", "cg", "-p", "mgpoly"] + small + SIZE)
    assert out.returncode == 1 and "goes with -t pcg only" in out.stderr.decode()
    out = run([crs, "-t", "pcg", "-p", "mgpol"] + small + SIZE)
    assert out.returncode == 1 and "Unknown preconditioner mgpol" in out.stderr.decode()
    for exe in ("sparseBench-CRS-HIP-SP", "sparseBench-SCS-HIP-SP"):
        out = run([os.path.join(BIN, exe), "-t", "pcg", "-p", "mgpoly"] + small + SIZE)
        assert out.returncode == 1 and "PCG: double precision only" in out.stderr.decode()
