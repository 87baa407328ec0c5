"""The Chebyshev-smoothed V-cycle's surface without a GPU: the new entry points are declared in include/sbhip.h,
exported by libsbhip.so, listed in capi.SYMBOLS and prototyped with their argument counts; the four drop-in libraries export
solvePCGMGPoly with the declared prototype; hostapi.PCG refuses a single-precision problem, a dinv, coarse_steps or galerkin with
another kind, and steps, coarse_steps, lmax or ratio out of range before it touches the library; mg_galerkin refuses what it
cannot coarsen; the driver's help and messages name -p mgpoly; loading initialises no device."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")

NEW = {"sb_pcg_create_mg_poly": 14, "sb_pcg_mg_poly_level_steps": 2, "sb_pcg_mg_poly_interval": 3, "sb_pcg_mg_poly_coeffs": 3,
       "sb_pcg_mg_poly_probe": 8, "sb_pcg_mg_poly_first_native": 9, "sb_pcg_mg_poly_first_launch": 2}


def test_mg_poly_symbols_declared_exported_listed_and_prototyped():
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
    assert L.sb_pcg_create_mg_poly.restype is ctypes.c_void_p and L.sb_pcg_mg_poly_level_steps.restype is ctypes.c_int
    assert L.sb_pcg_create_mg_poly.argtypes[10:] == [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double]
    assert L.sb_pcg_create_mg_poly.argtypes[:10] == L.sb_pcg_create_mg_p.argtypes  # the hierarchy as sb_pcg_create_mg_p takes it
    assert len(L.sb_pcg_create_poly.argtypes) == 7 and len(L.sb_pcg_create_mg_p.argtypes) == 10  # the existing kinds keep theirs
    whole = open(os.path.join(ROOT, "include", "sbhip.h")).read()
    assert re.search(r"\(below\), 4 Chebyshev polynomial,\s+5 Chebyshev-smoothed MG", whole)
    assert L.sb_is_initialized() == 0  # loading touched no device


@pytest.mark.parametrize("lib", ["libsparsebench_crs.so", "libsparsebench_scs.so", "libsparsebench_crs_sp.so", "libsparsebench_scs_sp.so"])
def test_dropin_libraries_export_solvePCGMGPoly(lib):
    from sparsebench_amd import hostapi
    hostapi.host()
    hostapi.host("single")
    d = ctypes.CDLL(os.path.join(LIB, lib))
    assert hasattr(d, "solvePCGMGPoly") and hasattr(d, "solvePCGMGFW") and hasattr(d, "solvePCGPoly")
    hdr = open(os.path.join(ROOT, "include", "sparsebench", "sparsebench.h")).read()
    assert re.search(r"\bint\s+solvePCGMGPoly\s*\(\s*Comm\s*\*\s*comm\s*,\s*Parameter\s*\*\s*param\s*,\s*Matrix\s*\*\s*m\s*\)\s*;", hdr)
    m = re.search(r"\bint\s+sbh_solve_pcg_mgpoly\s*\(([^)]*)\)", hdr)
    assert m and len(m.group(1).split(",")) == 10 and re.search(r"int\s+levels\s*,\s*int\s+steps\s*$", m.group(1))


def test_hostapi_pcg_refuses_before_the_library_is_touched():
    from sparsebench_amd import hostapi

    class Fake:  # never touched: the refusal comes first
        precision = "double"
        nr = 4
        filename = "generate"

        def rhs(self):
            raise AssertionError("the library was touched")

    class FakeSP(Fake):
        precision = "single"

    with pytest.raises(ValueError, match="double precision only"):
        hostapi.PCG(FakeSP(), precond="mgpoly")
    with pytest.raises(ValueError, match="precond='mgpoly' takes no dinv"):
        hostapi.PCG(Fake(), np.ones(4), precond="mgpoly", coarse=[])
    with pytest.raises(ValueError, match="not both"):
        hostapi.PCG(Fake(), precond="mgpoly", levels=2, coarse=[])
    for what in ("steps", "coarse_steps"):
        for bad in (0, -1, 17, 2.5, "3", True):
            with pytest.raises(ValueError, match="%s must be an integer from 1 to 16" % what):
                hostapi.PCG(Fake(), precond="mgpoly", coarse=[], **{what: bad})
    for lmax in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="lmax must be finite and positive"):
            hostapi.PCG(Fake(), precond="mgpoly", coarse=[], lmax=lmax)
    for ratio in (1.0, 0.5, 0.0, -4.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="ratio .* must be finite and greater than 1"):
            hostapi.PCG(Fake(), precond="mgpoly", coarse=[], ratio=ratio)
    for precond in ("jacobi", "sgs", "mg", "mgfw", "poly"):
        for kw in (dict(coarse_steps=2), dict(galerkin=True)):
            with pytest.raises(ValueError, match="coarse_steps and galerkin go with precond='mgpoly' only"):
                hostapi.PCG(Fake(), precond=precond, **kw)
    for precond in ("jacobi", "sgs", "mg", "mgfw"):
        with pytest.raises(ValueError, match="go with precond='poly' only, or with 'mgpoly'"):
            hostapi.PCG(Fake(), precond=precond, steps=2)
    with pytest.raises(ValueError, match="galerkin must be True or False"):
        hostapi.PCG(Fake(), precond="mgpoly", galerkin=1)
    with pytest.raises(ValueError, match="galerkin=True builds the coarse operators itself"):
        hostapi.PCG(Fake(), precond="mgpoly", galerkin=True, coarse=[])
    with pytest.raises(ValueError, match=r"precond='mgpoly' takes coarse=\[\(Problem, P, omega\), \.\.\.\]: entry 0"):
        hostapi.PCG(Fake(), precond="mgpoly", coarse=[(Fake(), None)])
    with pytest.raises(ValueError, match="omega of level 0 must be finite and positive"):
        hostapi.PCG(Fake(), precond="mgpoly", coarse=[(Fake(), None, 0.0)])
    not_generated = Fake()
    not_generated.filename = "some.mtx"
    with pytest.raises(ValueError, match="precond='mgpoly' needs the grid"):
        hostapi.PCG(not_generated, precond="mgpoly")
    for bad in ("mgcheb", "mg_poly", "MGPOLY", None):
        with pytest.raises(ValueError, match="precond must be 'jacobi' or 'sgs' or 'mg' or 'mgfw' or 'poly' or 'mgpoly'"):
            hostapi.PCG(Fake(), precond=bad)
    # in range: the refusals are passed and the library is reached
    with pytest.raises(AssertionError, match="the library was touched"):
        hostapi.PCG(Fake(), precond="mgpoly", coarse=[], steps=16, coarse_steps=1, lmax=1.5, ratio=1.0001)
    for name in ("precond", "steps", "level_steps", "interval", "coeffs", "levels", "level_rows", "mg_poly_probe", "apply", "apply_ms",
                 "precond_bytes", "solve", "start", "run_iters", "finish", "history", "solution", "dinv", "launches_per_body", "free"):
        assert callable(getattr(hostapi.PCG, name)), name


def test_mg_galerkin_refuses_what_it_cannot_coarsen():
    from sparsebench_amd import hostapi

    class Fake:
        precision, filename, nr, totalNr, dims = "double", "generate", 27, 27, (3, 3, 3)

    file_problem = Fake()
    file_problem.filename = "a.mtx"
    with pytest.raises(ValueError, match="mg_galerkin needs the grid"):
        hostapi.mg_galerkin(file_problem)
    two_ranks = Fake()
    two_ranks.totalNr = 54
    with pytest.raises(ValueError, match="one rank"):
        hostapi.mg_galerkin(two_ranks)
    sp = Fake()
    sp.precision = "single"
    with pytest.raises(ValueError, match="double precision only"):
        hostapi.mg_galerkin(sp)
    with pytest.raises(ValueError):  # 3 x 3 x 3 has no second level
        hostapi.mg_galerkin(Fake(), levels=2)
    assert "ImportError" in hostapi.mg_galerkin.__doc__ and "scipy" in hostapi.mg_galerkin.__doc__


def test_driver_help_and_messages_name_mgpoly():
    import driver_options as opts
    help_text = opts.help_text()
    assert re.search(r"-p mgpoly\b", help_text) and re.search(r"-p mgpoly.*-l.*-d.*Default 2", help_text, re.S)  # (the switch's two lines)
    assert re.search(r"-p <jacobi\|sgs>.*Default jacobi", help_text) and "-C <int>" in help_text  # the help text is still whole
    small, SIZE = ["-i", "10"], opts.SIZE
    # the defaults are solvePCGMGPoly's spec (the symbol itself runs in test_gpu_mg_poly_driver.py); -l and -d are the other path
    assert opts.accepted(["-t", "pcg", "-p", "mgpoly"] + small + SIZE).spec == (opts.KIND["mgpoly"], 0, 0, opts.COARSE["regenerated"])
    assert opts.accepted(["-t", "pcg", "-p", "mgpoly", "-l", "3"] + small + SIZE).spec == (opts.KIND["mgpoly"], 3, 0, 0)
    assert opts.accepted(["-t", "pcg", "-p", "mgpoly", "-d", "1"] + small + SIZE).spec == (opts.KIND["mgpoly"], 0, 1, 0)
    p = opts.accepted(["-t", "pcg", "-p", "mgpoly", "-C", "64", "-s", "256", "-l", "3", "-d", "2"] + small + SIZE)
    assert p.spec == (opts.KIND["mgpoly"], 3, 2, 0) and (p.scsC, p.scsSigma) == (64, 256)
    opts.refused(["-t", "pcg", "-p", "mgpoly", "-m", "tri.mtx"] + small, "-p mgpoly needs the grid")
    opts.refused(["-t", "pcg", "-p", "mgpoly", "-l", "5"] + small + SIZE, "5 levels would give a coarse dimension smaller than 2")
    opts.refused(["-t", "pcg", "-p", "mgpoly", "-l", "2", "-x", "15", "-y", "16", "-z", "16"] + small, "2 levels need every dimension divisible by 2")
    for bad in ("0", "17", "x"):
        opts.refused(["-t", "pcg", "-p", "mgpoly", "-d", bad] + small + SIZE, "-d <int> (the steps of -p poly or -p mgpoly) must be 1 to 16")
    opts.refused(["-t", "pcg", "-p", "mgfw", "-d", "2"] + small + SIZE, "-d <int> (the steps) goes with -p poly only, or with -p mgpoly\n")
    opts.refused(["-t", "pcg", "-p", "sgs", "-l", "2"] + small + SIZE, "-l <int> (the levels) goes with -p mg only, or with -p mgfw or -p mgpoly\n")
    opts.refused(["-t", "cg", "-p", "mgpoly"] + small + SIZE, "goes with -t pcg only")
    opts.refused(["-t", "pcg", "-p", "mgpol"] + small + SIZE, "Unknown preconditioner mgpol")
    opts.refused(["-t", "pcg", "-p", "mgpoly"] + small + SIZE, "PCG: double precision only", precision="single")
    assert opts.no_device_was_touched()
