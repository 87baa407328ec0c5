"""The surface of BiCGStab under a preconditioner plan without a GPU: the new entry points are declared in
include/sbhip.h, exported by libsbhip.so, listed in capi.SYMBOLS and prototyped; the four drop-in libraries export
solveBiCGStabPrecond with the declared prototype and the host library sbh_solve_bicgstab_precond; hostapi.BiCGStab's refusals that
come before the library is touched; the driver's help names -P and its refusals are in place; loading initialises no device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")
NEW = ["sb_bicgstab_create_pre", "sb_bicgstab_precond", "sb_bicgstab_plan_update_p_native", "sb_bicgstab_plan_update_s_native"]


def test_symbols_declared_exported_listed_and_prototyped():
    from sparsebench_amd import capi
    L = capi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbhip.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), "include/sbhip.h does not declare %s" % n
        assert hasattr(L, n), "libsbhip.so does not export %s" % n
        assert n in capi.SYMBOLS
        assert getattr(L, n).argtypes is not None, "capi.load() gives %s no prototype" % n
    assert len(L.sb_bicgstab_create_pre.argtypes) == 5 and len(L.sb_bicgstab_precond.argtypes) == 1
    assert len(L.sb_bicgstab_plan_update_p_native.argtypes) == 11 and len(L.sb_bicgstab_plan_update_s_native.argtypes) == 10
    assert re.search(r"sb_bicgstab_create_pre\s*\([^)]*const\s+sb_pcg\s*\*\s*M\s*\)", header)
    assert L.sb_is_initialized() == 0  # loading touched no device


@pytest.mark.parametrize("lib", ["libsparsebench_crs.so", "libsparsebench_scs.so", "libsparsebench_crs_sp.so", "libsparsebench_scs_sp.so"])
def test_dropin_libraries_export_solveBiCGStabPrecond(lib):
    from sparsebench_amd import hostapi
    hostapi.host()
    hostapi.host("single")
    d = ctypes.CDLL(os.path.join(LIB, lib))
    assert hasattr(d, "solveBiCGStabPrecond") and hasattr(d, "solveBiCGStab")
    hdr = open(os.path.join(ROOT, "include", "sparsebench", "sparsebench.h")).read()
    assert re.search(r"\bint\s+solveBiCGStabPrecond\s*\(\s*Comm\s*\*\s*comm\s*,\s*Parameter\s*\*\s*param\s*,\s*Matrix\s*\*\s*m\s*,\s*int\s+precond\s*\)\s*;",
                     hdr)
    assert re.search(r"\bint\s+sbh_solve_bicgstab_precond\s*\(\s*Comm\s*\*\s*comm\s*,\s*Parameter\s*\*\s*param\s*,\s*void\s*\*\s*dev_matrix\s*,"
                     r"\s*CG_UINT\s+nr\s*,\s*const\s+CG_UINT\s*\*\s*rowNnz\s*,\s*int\s+fmt\s*,\s*CG_UINT\s+C\s*,\s*CG_UINT\s+sigma\s*,\s*int\s+precond\s*,"
                     r"\s*int\s+levels\s*,\s*int\s+steps\s*,\s*int\s+galerkin\s*\)\s*;", hdr)
    h = ctypes.CDLL(os.path.join(LIB, "libsparsebench_host%s.so" % ("_sp" if lib.endswith("_sp.so") else "")))
    assert hasattr(h, "sbh_solve_bicgstab_precond")


def test_hostapi_refusals_before_the_library_and_methods():
    from sparsebench_amd import hostapi

    class FakeSP:  # never touched: the refusal comes first
        precision = "single"

        def rhs(self):
            raise AssertionError("the library was touched")

    for precond in hostapi.BiCGStab.PLANS:
        with pytest.raises(ValueError, match="double precision only"):
            hostapi.BiCGStab(FakeSP(), precond=precond)

    class Fake(FakeSP):
        precision = "double"
        nr = 27

    assert hostapi.BiCGStab.PLANS == ("sgs", "mg", "mgfw", "poly", "mgpoly")
    for precond in hostapi.BiCGStab.PLANS:
        with pytest.raises(ValueError, match="takes no dinv"):
            hostapi.BiCGStab(Fake(), precond=precond, dinv=[1.0] * 27)
    with pytest.raises(TypeError, match="go with precond 'sgs', 'mg', 'mgfw', 'poly' or 'mgpoly' only"):
        hostapi.BiCGStab(Fake(), precond="jacobi", steps=3)
    with pytest.raises(ValueError, match="precond must be 'none' or 'jacobi', or pass dinv"):
        hostapi.BiCGStab(Fake(), precond="ilu")  # the existing refusal stands
    with pytest.raises(ValueError, match="steps must be an integer from 1 to 16"):
        hostapi.BiCGStab(Fake(), precond="poly", steps=17)  # PCG's own checks, before it touches the library
    assert callable(hostapi.BiCGStab.precond)


def test_driver_help_names_P_and_the_refusals_are_in_place():
    import driver_options as opts
    help_text = opts.help_text()
    assert re.search(r"-P <sgs\|mg\|mgfw\|poly\|mgpoly>.*-t bicgstab", help_text)
    for whole in (r"-p <jacobi\|sgs>.*Default jacobi", r"-g\b.*Galerkin coarse operators.*-p mgpoly", r"-d <int>   Steps of -p poly",
                  r"-l <int>   Levels of -p mg", r"-C <int>", r"-s <int>"):
        assert re.search(whole, help_text), whole  # the help text is otherwise whole
    size, K, C = ["-x", "8", "-y", "8", "-z", "8", "-i", "10"], opts.KIND, opts.COARSE
    # every plan at its defaults is solveBiCGStabPrecond's spec (the symbol itself runs in test_gpu_bicgstab_precond_driver.py);
    # -l, -d, -g and -a are the other path
    for name in ("sgs", "mg", "mgfw", "poly", "mgpoly"):
        p = opts.accepted(["-t", "bicgstab", "-P", name] + size)
        assert p.type == opts.TYPE["bicgstab"] and p.byP == 1 and p.spec == (K[name], 0, 0, 0)
    for extra, spec in ((["-P", "mg", "-l", "2"], (K["mg"], 2, 0, 0)), (["-P", "mgfw", "-l", "3"], (K["mgfw"], 3, 0, 0)),
                        (["-P", "poly", "-d", "3"], (K["poly"], 0, 3, 0)), (["-P", "mgpoly", "-l", "2", "-d", "1"], (K["mgpoly"], 2, 1, 0)),
                        (["-P", "mgpoly", "-g", "-d", "1"], (K["mgpoly"], 0, 1, C["galerkin"])),
                        (["-P", "mgpoly", "-a", "-d", "2"], (K["mgpoly"], 0, 2, C["aggregation"]))):
        p = opts.accepted(["-t", "bicgstab"] + extra + size)
        assert p.byP == 1 and p.spec == spec, extra
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
        opts.refused(args + size, msg)
    opts.refused(["-t", "bicgstab", "-P", "poly"] + size, "BiCGStab: double precision only", precision="single")
    assert opts.no_device_was_touched()  # before the set-up: the parser has no way to a device
    solver = open(os.path.join(ROOT, "sparsebench_amd", "host", "sbh_solver.c")).read()
    assert solver.count("sb_pcg_create_sgs(") == solver.count("sb_pcg_create_poly(") == solver.count("sb_pcg_create_mg(") == 1  # one builder
    assert "sb_bicgstab_create_pre(" in solver
