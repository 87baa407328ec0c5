"""The surface of right-preconditioned GMRES(m) without a GPU: the new entry points are declared in include/sbhip.h,
exported by libsbhip.so, listed in capi.SYMBOLS and prototyped; the four drop-in libraries export solveGMRESPrecond with the
declared prototype and the host libraries sbh_solve_gmres_precond; hostapi.GMRES's refusals that come before the library is
touched; the driver's help names -P with -t gmres and its refusals are in place; loading initialises no device."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")
NEW = {"sb_gmres_create_pre": 6, "sb_gmres_create_dinv": 6, "sb_gmres_precond": 1, "sb_gmres_dinv": 2, "sb_gmres_pre_scale_native": 10,
       "sb_gmres_pre_multiupdate_native": 11, "sb_gmres_pre_step_native": 13}


def test_symbols_declared_exported_listed_and_prototyped():
    from sparsebench_amd import capi
    L = capi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbhip.h")).read(), flags=re.S)
    for n, nargs in NEW.items():
        assert re.search(r"\b%s\s*\(" % n, header), "include/sbhip.h does not declare %s" % n
        assert hasattr(L, n), "libsbhip.so does not export %s" % n
        assert n in capi.SYMBOLS
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == nargs, n
    assert re.search(r"sb_gmres\s*\*\s*sb_gmres_create_pre\s*\(\s*const\s+sb_matrix\s*\*\s*m\s*,\s*sb_halo\s*\*\s*halo\s*,\s*const\s+double\s*\*\s*"
                     r"b_host\s*,\s*const\s+double\s*\*\s*xexact_host\s*,\s*int\s+restart\s*,\s*const\s+sb_pcg\s*\*\s*M\s*\)\s*;", header)
    assert re.search(r"\bint\s+sb_gmres_precond\s*\(\s*const\s+sb_gmres\s*\*\s*s\s*\)\s*;", header)
    assert re.search(r"\bvoid\s+sb_gmres_dinv\s*\(\s*const\s+sb_gmres\s*\*\s*s\s*,\s*double\s*\*\s*dinv_host\s*\)\s*;", header)
    assert len(L.sb_gmres_create.argtypes) == 5  # the unpreconditioned entry is as it was
    assert L.sb_is_initialized() == 0  # loading touched no device


@pytest.mark.parametrize("lib", ["libsparsebench_crs.so", "libsparsebench_scs.so", "libsparsebench_crs_sp.so", "libsparsebench_scs_sp.so"])
def test_dropin_libraries_export_solveGMRESPrecond(lib):
    from sparsebench_amd import hostapi
    hostapi.host()
    hostapi.host("single")
    d = ctypes.CDLL(os.path.join(LIB, lib))
    assert hasattr(d, "solveGMRESPrecond") and hasattr(d, "solveGMRES")
    hdr = open(os.path.join(ROOT, "include", "sparsebench", "sparsebench.h")).read()
    assert re.search(r"\bint\s+solveGMRESPrecond\s*\(\s*Comm\s*\*\s*comm\s*,\s*Parameter\s*\*\s*param\s*,\s*Matrix\s*\*\s*m\s*,\s*int\s+restart\s*,"
                     r"\s*int\s+precond\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+sbh_solve_gmres_precond\s*\(\s*Comm\s*\*\s*comm\s*,\s*Parameter\s*\*\s*param\s*,\s*void\s*\*\s*dev_matrix\s*,"
                     r"\s*CG_UINT\s+nr\s*,\s*const\s+CG_UINT\s*\*\s*rowNnz\s*,\s*int\s+fmt\s*,\s*CG_UINT\s+C\s*,\s*CG_UINT\s+sigma\s*,\s*int\s+restart\s*,"
                     r"\s*int\s+precond\s*,\s*int\s+levels\s*,\s*int\s+steps\s*,\s*int\s+galerkin\s*\)\s*;", hdr)
    h = ctypes.CDLL(os.path.join(LIB, "libsparsebench_host%s.so" % ("_sp" if lib.endswith("_sp.so") else "")))
    assert hasattr(h, "sbh_solve_gmres_precond") and hasattr(h, "sbh_solve_gmres")


def test_hostapi_refusals_before_the_library_and_methods():
    from sparsebench_amd import hostapi

    class FakeSP:  # never touched: the refusal comes first
        precision = "single"

        def rhs(self):
            raise AssertionError("the library was touched")

    for precond in ("none", "jacobi") + hostapi.GMRES.PLANS:
        with pytest.raises(ValueError, match="double precision only"):
            hostapi.GMRES(FakeSP(), precond=precond)

    class Fake(FakeSP):
        precision = "double"
        nr = 27

    sig = inspect.signature(hostapi.GMRES.__init__)
    assert list(sig.parameters)[:6] == ["self", "problem", "restart", "fused", "precond", "dinv"]
    assert [sig.parameters[n].default for n in ("restart", "fused", "precond", "dinv")] == [30, True, "none", None]
    assert hostapi.GMRES.PLANS == ("sgs", "mg", "mgfw", "poly", "mgpoly")
    for precond in hostapi.GMRES.PLANS:
        with pytest.raises(ValueError, match="takes no dinv"):
            hostapi.GMRES(Fake(), precond=precond, dinv=[1.0] * 27)
    with pytest.raises(TypeError, match="go with precond 'sgs', 'mg', 'mgfw', 'poly' or 'mgpoly' only"):
        hostapi.GMRES(Fake(), precond="jacobi", steps=3)
    with pytest.raises(TypeError, match="go with precond 'sgs', 'mg', 'mgfw', 'poly' or 'mgpoly' only"):
        hostapi.GMRES(Fake(), steps=3)
    with pytest.raises(ValueError, match="precond must be 'none', 'jacobi', 'sgs', 'mg', 'mgfw', 'poly', 'mgpoly' or a PCG handle"):
        hostapi.GMRES(Fake(), precond="ilu")
    with pytest.raises(ValueError, match="it goes with no other precond"):
        hostapi.GMRES(Fake(), precond="jacobi", dinv=[1.0] * 27)
    with pytest.raises(ValueError, match="dinv must hold nr = 27 doubles"):
        hostapi.GMRES(Fake(), dinv=[1.0] * 26)
    for bad in (0.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="finite and non-zero"):
            hostapi.GMRES(Fake(), dinv=[1.0] * 26 + [bad])
    with pytest.raises(ValueError, match="steps must be an integer from 1 to 16"):
        hostapi.GMRES(Fake(), precond="poly", steps=17)  # PCG's own checks, before it touches the library
    assert callable(hostapi.GMRES.precond) and callable(hostapi.GMRES.dinv)
    for name in ("history", "solve", "launches_per_step", "run_steps", "restart"):
        assert callable(getattr(hostapi.GMRES, name))


def test_driver_help_names_P_for_gmres_and_the_refusals_are_in_place():
    import driver_options as opts
    help_text = opts.help_text()
    assert re.search(r"-P <sgs\|mg\|mgfw\|poly\|mgpoly>.*-t bicgstab", help_text)  # the line of before
    assert re.search(r"-t gmres.*-P jacobi", help_text)
    assert re.search(r"-r <int>   GMRES restart length", help_text)
    size, K, C = ["-x", "8", "-y", "8", "-z", "8", "-i", "10"], opts.KIND, opts.COARSE
    # every preconditioner at its defaults is solveGMRESPrecond's spec (the symbol itself runs in test_gpu_gmres_precond_driver.py);
    # -l, -d, -g and -a are the other path; without -P: solveGMRES's call of before
    for name in ("jacobi", "sgs", "mg", "mgfw", "poly", "mgpoly"):
        p = opts.accepted(["-t", "gmres", "-r", "10", "-P", name] + size)
        assert p.type == opts.TYPE["gmres"] and p.byP == 1 and p.spec == (K[name], 0, 0, 0) and p.restart == 10
    for extra, spec in ((["-P", "mg", "-l", "2"], (K["mg"], 2, 0, 0)), (["-P", "mgfw", "-l", "3"], (K["mgfw"], 3, 0, 0)),
                        (["-P", "poly", "-d", "3"], (K["poly"], 0, 3, 0)), (["-P", "mgpoly", "-l", "2", "-d", "1"], (K["mgpoly"], 2, 1, 0)),
                        (["-P", "mgpoly", "-g", "-d", "1"], (K["mgpoly"], 0, 1, C["galerkin"])),
                        (["-P", "mgpoly", "-a", "-d", "2"], (K["mgpoly"], 0, 2, C["aggregation"]))):
        p = opts.accepted(["-t", "gmres"] + extra + size)
        assert p.byP == 1 and p.spec == spec and p.restart == 30, extra
    p = opts.accepted(["-t", "gmres", "-r", "12"] + size)
    assert p.type == opts.TYPE["gmres"] and not p.byP and p.spec == (K[None], 0, 0, 0) and p.restart == 12
    opts.refused(["-t", "cg", "-P", "sgs"] + size, "-P <sgs|mg|mgfw|poly|mgpoly> (the preconditioner of BiCGStab) goes with -t bicgstab only, or as "
                 "-P <jacobi|sgs|mg|mgfw|poly|mgpoly> with -t gmres\n")
    for args, msg in ((["-t", "gmres", "-p", "sgs"], "goes with -t pcg only"),
                      (["-t", "pcg", "-P", "sgs"], "goes with -t bicgstab only"),
                      (["-P", "poly"], "goes with -t bicgstab only"),
                      (["-t", "pcg", "-P", "jacobi"], "Unknown preconditioner jacobi (-P <sgs|mg|mgfw|poly|mgpoly>)"),
                      (["-t", "bicgstab", "-P", "jacobi"], "Unknown preconditioner jacobi (-P <sgs|mg|mgfw|poly|mgpoly>)"),  # refused as before
                      (["-t", "gmres", "-P", "ilu"], "Unknown preconditioner ilu"),
                      (["-t", "gmres", "-P", "sgs", "-d", "3"], "-d <int> (the steps) goes with -p poly only"),
                      (["-t", "gmres", "-P", "jacobi", "-l", "2"], "-l <int> (the levels) goes with -p mg only"),
                      (["-t", "gmres", "-P", "poly", "-g"], "-g (Galerkin coarse operators) goes with -p mgpoly only"),
                      (["-t", "gmres", "-l", "2"], "-l <int> (the levels) goes with -p mg only"),
                      (["-t", "gmres", "-P", "mgpoly", "-a", "-g"], "it does not go with -g"),
                      (["-t", "gmres", "-P", "mgpoly", "-m", "some.mtx"], "-P mgpoly needs the grid")):
        opts.refused(args + size, msg)
    opts.refused(["-t", "gmres", "-P", "poly"] + size, "GMRES: double precision only", precision="single")
    assert opts.no_device_was_touched()  # before the set-up: the parser has no way to a device
    solver = open(os.path.join(ROOT, "sparsebench_amd", "host", "sbh_solver.c")).read()
    assert solver.count("sb_pcg_create_sgs(") == solver.count("sb_pcg_create_poly(") == solver.count("sb_pcg_create_mg(") == 1  # one builder
    assert "sb_gmres_create_pre(" in solver and solver.count("sb_gmres_solve(") == 1  # one runner for both
