"""`-t pcg -p mgfw` from the benchmark drivers and solvePCGMGFW through a drop-in library: the preconditioner line,
the iteration count and every printed residual of tests/golden/mg_fw_hist.json at 16^3, in the natural order (CRS) and in a
permuted one (-s 256), at -l 3 and at the auto depth; `-p mg` prints what it printed; the switches' refusals."""
import math
import os
import re
import subprocess

import pytest

import mg_cases
import mg_fw_cases as cases
from conftest import load_json

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sparsebench_amd", "bin")
SIZE = ["-x", "16", "-y", "16", "-z", "16"]
LINE = r"Preconditioner: MG \(V-cycle, full-weighting transfers, multicolour SGS smoother\), levels = %d, nC = %d"


def run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def check_output(txt, e, head=r"^Test type: PCG\n(Generate .*\n)*"):
    """the golden case's k, and with -i 19 (a line per iteration) the residual every iteration starts from, the last included;
    head: what stands before the preconditioner's line (the driver's own lines; "^" for a caller that prints none)"""
    rr = [float.fromhex(v) for v in e["rr"]]
    assert 1 < e["k"] < 19 and len(rr) == e["k"] - 1
    assert re.search(head + LINE % (e["L"], e["nC"][0]) + "$", txt, re.M), txt[-2000:]
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
def test_driver_runs_mgfw_pcg(gpu, exe, order, names):
    golden = load_json("mg_fw_hist.json")["cases"]
    printed = []
    for levels, name in zip((["-l", "3"], []), names):  # without -l: auto, HPCG's depth at 16^3, through solvePCGMGFW
        e, c = golden[name], cases.CASES[name]
        assert (c["C"], c["sigma"]) == ((64, 256) if order else (64, 1))
        out = run([os.path.join(BIN, exe), "-t", "pcg", "-p", "mgfw"] + order + levels + ["-i", "19", "-e", "%.17g" % float.fromhex(e["eps"])] + SIZE)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        printed.append(check_output(out.stdout.decode(), e))
    assert [a for a, b in zip(*printed) if a != b]  # the depth shows in the printed residuals, in the natural order too


def test_solvePCGMGFW_through_the_dropin_library(gpu, tmp_path):
    """the symbol, run by a C caller of its own, and the driver at the defaults: both the golden case's lines"""
    import ctypes
    import driver_options
    from sparsebench_amd import hostapi
    hostapi.host()
    e = load_json("mg_fw_hist.json")["cases"]["hpcg16_crs_L4"]
    for fmt, exe in (("crs", "sparseBench-CRS-HIP"), ("scs", "sparseBench-SCS-HIP")):  # (Sell-64-1, the default: the natural order)
        d = ctypes.CDLL(os.path.join(ROOT, "sparsebench_amd", "lib", "libsparsebench_%s.so" % fmt))
        assert hasattr(d, "solvePCGMGFW")
        assert "libsparsebench_%s.so" % fmt in run(["ldd", os.path.join(BIN, exe)]).stdout.decode()
        called, k = driver_options.run_dropin_symbol(tmp_path, fmt.upper(), "SOLVER_PCG_MGFW", ["16", "19", "%.17g" % float.fromhex(e["eps"])])
        assert k == e["k"]
        check_output(called, e, head="^")
        txt = run([os.path.join(BIN, exe), "-t", "pcg", "-p", "mgfw", "-i", "19", "-e", "%.17g" % float.fromhex(e["eps"])] + SIZE).stdout.decode()
        check_output(txt, e)


def test_mg_output_is_unchanged(gpu):
    e, c = load_json("mg_hist.json")["cases"]["hpcg16_crs_L4"], mg_cases.CASES["hpcg16_crs_L4"]
    out = run([os.path.join(BIN, "sparseBench-CRS-HIP"), "-t", "pcg", "-p", "mg", "-i", str(c["itermax"]), "-e", "%.17g" % float.fromhex(e["eps"])] + SIZE)
    txt = out.stdout.decode()
    assert out.returncode == 0 and "full-weighting" not in txt
    assert re.search(r"^Preconditioner: MG \(V-cycle, multicolour SGS smoother\), levels = 4, nC = %d$" % e["nC"][0], txt, re.M), txt[-2000:]
    assert re.search(r"^Solution performed %d iterations" % e["k"], txt, re.M)
    rr = [float.fromhex(v) for v in e["rr"]]
    assert "Initial Residual = %E" % math.sqrt(rr[0]) in txt and "Iteration = 15 Residual = %E" % math.sqrt(rr[14]) in txt


def test_switch_refusals(gpu, tmp_path):
    crs = os.path.join(BIN, "sparseBench-CRS-HIP")
    small = ["-i", "10"]
    help_text = run([crs, "-h"]).stdout.decode()
    assert re.search(r"-p mgfw\b", help_text) and re.search(r"-p mg\b", help_text) and "-l <int>" in help_text
    mtx = tmp_path / "tri.mtx"
    mg_cases.tridiagonal(str(mtx), 20, 4.0)
    out = run([crs, "-t", "pcg", "-p", "mgfw", "-m", str(mtx)] + small)
    assert out.returncode == 1 and "-p mgfw needs the grid" in out.stderr.decode(), out.stderr.decode()
    out = run([crs, "-t", "pcg", "-p", "mgfw", "-l", "5"] + small + SIZE)
    assert out.returncode == 1 and "5 levels would give a coarse dimension smaller than 2" in out.stderr.decode()
    out = run([crs, "-t", "pcg", "-p", "mgfw", "-l", "2", "-x", "15", "-y", "16", "-z", "16"] + small)
    assert out.returncode == 1 and "2 levels need every dimension divisible by 2" in out.stderr.decode()
    out = run([crs, "-t", "cg", "-p", "mgfw"] + small + SIZE)
    assert out.returncode == 1 and "goes with -t pcg only" in out.stderr.decode()
    out = run([crs, "-t", "pcg", "-p", "mgfx"] + small + SIZE)
    assert out.returncode == 1 and "Unknown preconditioner mgfx" in out.stderr.decode()
    for exe in ("sparseBench-CRS-HIP-SP", "sparseBench-SCS-HIP-SP"):
        out = run([os.path.join(BIN, exe), "-t", "pcg", "-p", "mgfw"] + small + SIZE)
        assert out.returncode == 1 and "PCG: double precision only" in out.stderr.decode()
