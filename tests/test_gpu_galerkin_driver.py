"""`-t pcg -p mgpoly -g` from the benchmark drivers and solvePCGMGPolyGalerkin through a drop-in library: the
preconditioner line with "Galerkin coarse operators" in it, the line with the products' device milliseconds per level, and the
iteration count and every printed residual of the Galerkin cases of tests/golden/mg_poly_hist.json at 16^3, in the natural order
(CRS) and in a permuted one (-C 64 -s 256); without -g the driver prints what it printed; -g without -p mgpoly is refused with
status 1 before the set-up."""
import ctypes
import os
import re
import subprocess

import pytest

import mg_poly_cases as cases
from conftest import load_json
from test_gpu_mg_poly_driver import check_output, LINE as PLAIN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sparsebench_amd", "bin")
SIZE = ["-x", "16", "-y", "16", "-z", "16"]
GLINE = PLAIN.replace(r" smoother\)", r" smoother, Galerkin coarse operators\)")
MS = r"^Galerkin products P\^T A P on the device, ms \(A P \+ P\^T \(A P\)\):%s$"


def run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def check_galerkin_output(txt, e, steps, levels):
    assert "Galerkin coarse operators" in GLINE
    plain = txt.replace(", Galerkin coarse operators)", ")")
    lines = check_output("\n".join(l for l in plain.split("\n") if not l.startswith("Galerkin products")), e, steps)
    iv = tuple(re.escape("%.6g" % float.fromhex(v)) for v in e["intervals"][0])
    assert re.search("^" + GLINE % ((e["L"], steps) + iv) + "$", txt, re.M), txt[-2000:]
    per_level = ",".join(r" level %d: \d+\.\d{3} \+ \d+\.\d{3}" % l for l in range(1, levels))
    assert re.search(MS % per_level, txt, re.M), txt[-2000:]
    return lines


@pytest.mark.parametrize("exe,order,name", [
    ("sparseBench-CRS-HIP", [], "hpcg16_crs_L3_galerkin"),
    ("sparseBench-SCS-HIP", ["-C", "64", "-s", "256"], "hpcg16_sell_64_256_L3_galerkin")])
def test_driver_runs_mgpoly_pcg_on_galerkin_operators(gpu, exe, order, name):
    e, c = load_json("mg_poly_hist.json")["cases"][name], cases.CASES[name]
    assert c["galerkin"] and c["levels"] == 3 and (c["C"], c["sigma"]) == ((64, 256) if order else (64, 1))
    out = run([os.path.join(BIN, exe), "-t", "pcg", "-p", "mgpoly", "-g", "-l", "3"] + order + ["-i", "19", "-e", "%.17g" % float.fromhex(e["eps"])] + SIZE)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    with_g = check_galerkin_output(out.stdout.decode(), e, 2, 3)
    # without -g: the regenerated hierarchy's lines, as before
    r = load_json("mg_poly_hist.json")["cases"][name[:-len("_galerkin")]]
    out = run([os.path.join(BIN, exe), "-t", "pcg", "-p", "mgpoly", "-l", "3"] + order + ["-i", "19", "-e", "%.17g" % float.fromhex(r["eps"])] + SIZE)
    assert out.returncode == 0 and "Galerkin" not in out.stdout.decode()
    assert check_output(out.stdout.decode(), r, 2) != with_g


def test_solvePCGMGPolyGalerkin_through_the_dropin_library(gpu, tmp_path):
    """the symbol, run by a C caller of its own, and the driver with -g at the defaults: both the golden count's depth and k"""
    import driver_options
    from sparsebench_amd import hostapi
    hostapi.host()
    count = load_json("mg_poly_hist.json")["counts"]["hpcg16_galerkin"]  # the deepest hierarchy, 2 steps, natural order
    assert cases.COUNT_CASES["hpcg16_galerkin"]["eps_rel"] == cases.CASES["hpcg16_crs_L3_galerkin"]["eps_rel"]  # the same eps: 1e-10 ||b||
    eps = float.fromhex(load_json("mg_poly_hist.json")["cases"]["hpcg16_crs_L3_galerkin"]["eps"])
    for fmt, exe in (("crs", "sparseBench-CRS-HIP"), ("scs", "sparseBench-SCS-HIP")):  # (Sell-64-1, the default: the natural order)
        d = ctypes.CDLL(os.path.join(ROOT, "sparsebench_amd", "lib", "libsparsebench_%s.so" % fmt))
        assert hasattr(d, "solvePCGMGPolyGalerkin")
        called, k = driver_options.run_dropin_symbol(tmp_path, fmt.upper(), "SOLVER_PCG_MGPOLY_GALERKIN", ["16", "19", "%.17g" % eps])
        assert k == count["k"]
        out = run([os.path.join(BIN, exe), "-t", "pcg", "-p", "mgpoly", "-g", "-i", "19", "-e", "%.17g" % eps] + SIZE)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        for txt in (called, out.stdout.decode()):
            assert re.search(r"^Preconditioner: MG .*Galerkin coarse operators\), levels = %d, steps = 2," % count["L"], txt, re.M), txt[-2000:]
            assert re.search(MS % ",".join(r" level %d: \d+\.\d{3} \+ \d+\.\d{3}" % l for l in range(1, count["L"])), txt, re.M), txt[-2000:]
            assert re.search(r"^Solution performed %d iterations" % count["k"], txt, re.M), txt[-2000:]
            assert "Difference between computed and exact  = 0.0000" in txt
        residuals = [[l for l in t.split("\n") if "Residual = " in l] for t in (called, out.stdout.decode())]
        assert len(residuals[0]) == count["k"] and residuals[0] == residuals[1]  # (-i 19: a line per iteration)


def test_g_is_refused_without_mgpoly_before_the_set_up(gpu):
    crs = os.path.join(BIN, "sparseBench-CRS-HIP")
    help_text = run([crs, "-h"]).stdout.decode()
    assert re.search(r"^\s+-g\s+Galerkin coarse operators", help_text, re.M)
    for args in (["-t", "pcg", "-p", "mgfw", "-g"], ["-t", "pcg", "-g"], ["-g"], ["-t", "pcg", "-p", "poly", "-g"]):
        out = run([crs] + args + ["-i", "10"] + SIZE)
        assert out.returncode == 1 and "-g (Galerkin coarse operators) goes with -p mgpoly only" in out.stderr.decode(), args
        assert "Setup took" not in out.stdout.decode() and "Generate" not in out.stdout.decode()
    for exe in ("sparseBench-CRS-HIP-SP", "sparseBench-SCS-HIP-SP"):
        out = run([os.path.join(BIN, exe), "-t", "pcg", "-p", "mgpoly", "-g", "-i", "10"] + SIZE)
        assert out.returncode == 1 and "PCG: double precision only" in out.stderr.decode()
