"""The BiCGStab surface without a GPU: the new entry points are declared in include/sbhip.h, exported by libsbhip.so, listed in
capi.SYMBOLS and prototyped; the four drop-in libraries export solveBiCGStab with the declared prototype; hostapi.BiCGStab
refuses a single-precision problem before it touches the library; the driver's help names the type; loading initialises no
device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")

NEW = ["sb_bicgstab_create", "sb_bicgstab_free", "sb_bicgstab_solve", "sb_bicgstab_start", "sb_bicgstab_run_iters", "sb_bicgstab_finish",
       "sb_bicgstab_history", "sb_bicgstab_solution", "sb_bicgstab_check_residual", "sb_bicgstab_dinv", "sb_bicgstab_launches_per_body",
       "sb_bicgstab_loop_ms", "sb_bicgstab_counters", "sb_bicgstab_update_p_native", "sb_bicgstab_update_s_native",
       "sb_bicgstab_dot2_native", "sb_bicgstab_update_xr_native", "sb_bicgstab_reduce_native", "sb_bicgstab_launch"]


def test_bicgstab_symbols_declared_exported_listed_and_prototyped():
    from sparsebench_amd import capi
    L = capi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbhip.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), "include/sbhip.h does not declare %s" % n
        assert hasattr(L, n), "libsbhip.so does not export %s" % n
        assert n in capi.SYMBOLS
        assert getattr(L, n).argtypes is not None, "capi.load() gives %s no prototype" % n
    assert len(L.sb_bicgstab_create.argtypes) == 6 and len(L.sb_bicgstab_history.argtypes) == 4
    assert len(L.sb_bicgstab_update_xr_native.argtypes) == 12 and len(L.sb_bicgstab_update_p_native.argtypes) == 8
    assert L.sb_is_initialized() == 0  # loading touched no device


@pytest.mark.parametrize("lib", ["libsparsebench_crs.so", "libsparsebench_scs.so", "libsparsebench_crs_sp.so", "libsparsebench_scs_sp.so"])
def test_dropin_libraries_export_solveBiCGStab(lib):
    from sparsebench_amd import hostapi
    hostapi.host()
    hostapi.host("single")
    d = ctypes.CDLL(os.path.join(LIB, lib))
    assert hasattr(d, "solveBiCGStab") and hasattr(d, "solvePCG")
    hdr = open(os.path.join(ROOT, "include", "sparsebench", "sparsebench.h")).read()
    assert re.search(r"\bint\s+solveBiCGStab\s*\(\s*Comm\s*\*\s*comm\s*,\s*Parameter\s*\*\s*param\s*,\s*Matrix\s*\*\s*m\s*\)\s*;", hdr)


def test_hostapi_bicgstab_refuses_single_precision_and_has_its_methods():
    from sparsebench_amd import hostapi

    class FakeSP:  # never touched: the refusal comes first
        precision = "single"

        def rhs(self):
            raise AssertionError("the library was touched")

    with pytest.raises(ValueError, match="double precision only"):
        hostapi.BiCGStab(FakeSP())
    with pytest.raises(ValueError, match="double precision only"):
        hostapi.BiCGStab(FakeSP(), precond="jacobi")
    for name in ("solve", "start", "run_iters", "finish", "history", "solution", "check_residual", "dinv", "launches_per_body",
                 "loop_ms", "counters", "free"):
        assert callable(getattr(hostapi.BiCGStab, name)), name
    assert hostapi.BiCGStab.HISTORIES == ("rr", "rho", "rv", "ts", "tt")


def test_driver_help_names_bicgstab_and_the_sp_drivers_refuse_it():
    import driver_options as opts
    help_text = opts.help_text()
    assert re.search(r"-t <bench type>.*\bbicgstab\b", help_text, re.S) and re.search(r"-t <bench type>.*\bpcg\b", help_text)  # (its two lines)
    size = ["-x", "8", "-y", "8", "-z", "8", "-i", "10"]
    p = opts.accepted(["-t", "bicgstab"] + size)
    assert p.type == opts.TYPE["bicgstab"] and p.spec == (opts.KIND[None], 0, 0, 0) and not p.byP  # no -P: solveBiCGStab's own diagonal
    opts.refused(["-t", "bicgstab"] + size, "BiCGStab: double precision only\n", precision="single")
    opts.refused(["-t", "cheb"] + size, "Unknown solver type cheb\n", stream="stdout")  # still an unknown type
    opts.refused(["-t", "bicgstab", "-n", "2"] + size, "-t cg only")
    assert opts.no_device_was_touched()
    solver = open(os.path.join(ROOT, "sparsebench_amd", "host", "sbh_solver.c")).read()
    assert "sbh_solve_bicgstab" in solver and "BiCGStab: double precision only" in solver
