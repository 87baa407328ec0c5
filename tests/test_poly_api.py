"""The polynomial preconditioner's surface without a GPU: the new entry points are declared in include/sbhip.h,
exported by libsbhip.so, listed in capi.SYMBOLS and prototyped with their argument counts; the four drop-in libraries export
solvePCGPoly with the declared prototype; hostapi.PCG refuses a single-precision problem, a dinv / levels / coarse argument and
steps, lmax or ratio out of range before it touches the library; the driver's help names -p poly and -d; loading initialises no
device."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")

NEW = {"sb_pcg_create_poly": 7, "sb_pcg_poly_steps": 1, "sb_pcg_poly_interval": 2, "sb_pcg_poly_coeffs": 2, "sb_pcg_poly_rowbound": 2,
       "sb_pcg_poly_update_r_native": 12, "sb_pcg_poly_step_native": 10, "sb_pcg_poly_step_launch": 2}


def test_poly_symbols_declared_exported_listed_and_prototyped():
    from sparsebench_amd import capi
    L = capi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbhip.h")).read(), flags=re.S)
    for n, nargs in NEW.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % n, header)
        assert m, "include/sbhip.h does not declare %s" % n
        assert len(m.group(1).split(",")) == nargs, "include/sbhip.h declares %s with other arguments" % n
        assert hasattr(L, n), "libsbhip.so does not export %s" % n
        assert n in capi.SYMBOLS
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == nargs, "capi.load() prototypes %s wrongly" % n
    assert L.sb_pcg_create_poly.restype is ctypes.c_void_p and L.sb_pcg_poly_steps.restype is ctypes.c_int
    assert L.sb_pcg_create_poly.argtypes[4:] == [ctypes.c_int, ctypes.c_double, ctypes.c_double]
    assert len(L.sb_pcg_create.argtypes) == 5 and len(L.sb_pcg_create_sgs.argtypes) == 4  # the existing kinds keep theirs
    whole = open(os.path.join(ROOT, "include", "sbhip.h")).read()
    assert "0 diagonal, 1 SGS, 2 MG, 3 MG with full-weighting transfers (below)" in whole and re.search(r"\(below\), 4 ", whole)
    assert L.sb_is_initialized() == 0  # loading touched no device


@pytest.mark.parametrize("lib", ["libsparsebench_crs.so", "libsparsebench_scs.so", "libsparsebench_crs_sp.so", "libsparsebench_scs_sp.so"])
def test_dropin_libraries_export_solvePCGPoly(lib):
    from sparsebench_amd import hostapi
    hostapi.host()
    hostapi.host("single")
    d = ctypes.CDLL(os.path.join(LIB, lib))
    assert hasattr(d, "solvePCGPoly") and hasattr(d, "solvePCGSGS") and hasattr(d, "solvePCG")
    hdr = open(os.path.join(ROOT, "include", "sparsebench", "sparsebench.h")).read()
    assert re.search(r"\bint\s+solvePCGPoly\s*\(\s*Comm\s*\*\s*comm\s*,\s*Parameter\s*\*\s*param\s*,\s*Matrix\s*\*\s*m\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+sbh_solve_pcg_poly\s*\(", hdr)


def test_hostapi_pcg_refuses_before_the_library_is_touched():
    from sparsebench_amd import hostapi

    class Fake:  # never touched: the refusal comes first
        precision = "double"
        nr = 4

        def rhs(self):
            raise AssertionError("the library was touched")

    class FakeSP(Fake):
        precision = "single"

    with pytest.raises(ValueError, match="double precision only"):
        hostapi.PCG(FakeSP(), precond="poly")
    with pytest.raises(ValueError, match="takes no dinv"):
        hostapi.PCG(Fake(), np.ones(4), precond="poly")
    with pytest.raises(ValueError, match="levels and coarse go with precond='mg' only"):
        hostapi.PCG(Fake(), precond="poly", levels=2)
    with pytest.raises(ValueError, match="levels and coarse go with precond='mg' only"):
        hostapi.PCG(Fake(), precond="poly", coarse=[])
    for steps in (0, -1, 17, 2.5, "3", True):
        with pytest.raises(ValueError, match="steps must be an integer from 1 to 16"):
            hostapi.PCG(Fake(), precond="poly", steps=steps)
    for lmax in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="lmax must be finite and positive"):
            hostapi.PCG(Fake(), precond="poly", lmax=lmax)
    for ratio in (1.0, 0.5, 0.0, -4.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="ratio .* must be finite and greater than 1"):
            hostapi.PCG(Fake(), precond="poly", ratio=ratio)
    for precond in ("jacobi", "sgs", "mg"):
        for kw in (dict(steps=3), dict(lmax=2.0), dict(ratio=16.0)):
            with pytest.raises(ValueError, match="go with precond='poly' only"):
                hostapi.PCG(Fake(), precond=precond, **kw)
    for bad in ("cheb", "chebyshev", "POLY", None, ""):
        with pytest.raises(ValueError, match="precond must be 'jacobi' or 'sgs' or 'mg' or 'mgfw' or 'poly'"):
            hostapi.PCG(Fake(), precond=bad)
    # in range: the refusals are passed and the library is reached
    with pytest.raises(AssertionError, match="the library was touched"):
        hostapi.PCG(Fake(), precond="poly", steps=16, lmax=1.5, ratio=1.0001)
    for name in ("precond", "steps", "interval", "coeffs", "rowbound", "apply", "apply_ms", "precond_bytes", "solve", "start",
                 "run_iters", "finish", "history", "solution", "dinv", "launches_per_body", "counters", "free"):
        assert callable(getattr(hostapi.PCG, name)), name


def test_driver_help_names_the_polynomial_switches():
    import driver_options as opts
    help_text = opts.help_text()
    assert re.search(r"-p poly\b", help_text) and re.search(r"-d <int>.*-p poly.*Default 3", help_text)
    assert re.search(r"-p <jacobi\|sgs>.*Default jacobi", help_text) and "-C <int>" in help_text  # the help text is still whole
    small = ["-x", "8", "-y", "8", "-z", "8", "-i", "10"]
    assert opts.accepted(["-t", "pcg", "-p", "poly"] + small).spec == (opts.KIND["poly"], 0, 0, 0)
    assert opts.accepted(["-t", "pcg", "-p", "poly", "-d", "2"] + small).spec == (opts.KIND["poly"], 0, 2, 0)
    for extra in (["-t", "pcg"], ["-t", "pcg", "-p", "jacobi"], ["-t", "pcg", "-p", "sgs"], ["-t", "pcg", "-p", "mg"], ["-t", "cg"], []):
        opts.refused(["-d", "2"] + extra + small, "-d <int> (the steps) goes with -p poly only")
    for bad in ("0", "17", "-3", "x"):
        opts.refused(["-t", "pcg", "-p", "poly", "-d", bad] + small, "must be 1 to 16, got %s\n" % bad)
    opts.refused(["-p", "poly"] + small, "goes with -t pcg only")  # the default type is cg
    opts.refused(["-t", "pcg", "-p", "poly", "-l", "2"] + small, "goes with -p mg only")
    opts.refused(["-t", "pcg", "-p", "cheb"] + small, "Unknown preconditioner cheb")
    opts.refused(["-t", "cheb"] + small, "Unknown solver type cheb\n", stream="stdout")  # still an unknown type
    opts.refused(["-t", "pcg", "-p", "poly"] + small, "PCG: double precision only", precision="single")
    assert opts.no_device_was_touched()
