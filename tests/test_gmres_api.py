"""The GMRES surface without a GPU: the new entry points are declared in include/sbhip.h, exported by libsbhip.so and
listed in capi.SYMBOLS; the drop-in libraries export solveGMRES; hostapi.GMRES refuses a single-precision problem before it
touches the library."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")

NEW = ["sb_gmres_create", "sb_gmres_free", "sb_gmres_set_fused", "sb_gmres_restart", "sb_gmres_launches_per_step",
       "sb_gmres_solve", "sb_gmres_start", "sb_gmres_run_steps", "sb_gmres_finish", "sb_gmres_history", "sb_gmres_solution",
       "sb_gmres_check_residual", "sb_gmres_loop_ms", "sb_gmres_counters", "sb_multidot", "sb_multiaxpy_sub"]


def test_gmres_symbols_declared_exported_and_listed():
    from sparsebench_amd import capi
    L = capi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbhip.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), "include/sbhip.h does not declare %s" % n
        assert hasattr(L, n), "libsbhip.so does not export %s" % n
        assert n in capi.SYMBOLS
    assert L.sb_is_initialized() == 0  # loading touched no device


@pytest.mark.parametrize("lib", ["libsparsebench_crs.so", "libsparsebench_scs.so", "libsparsebench_crs_sp.so", "libsparsebench_scs_sp.so"])
def test_dropin_libraries_export_solveGMRES(lib):
    from sparsebench_amd import hostapi
    hostapi.host()
    hostapi.host("single")
    d = ctypes.CDLL(os.path.join(LIB, lib))
    assert hasattr(d, "solveGMRES")
    hdr = open(os.path.join(ROOT, "include", "sparsebench", "sparsebench.h")).read()
    assert re.search(r"\bint\s+solveGMRES\s*\(", hdr)


def test_hostapi_gmres_refuses_single_precision():
    from sparsebench_amd import hostapi

    class FakeSP:  # never touched: the refusal comes first
        precision = "single"

        def rhs(self):
            raise AssertionError("the library was touched")

    with pytest.raises(ValueError, match="double precision only"):
        hostapi.GMRES(FakeSP())
    for name in ("solve", "start", "run_steps", "finish", "history", "solution", "check_residual", "launches_per_step",
                 "counters", "loop_ms", "free"):
        assert callable(getattr(hostapi.GMRES, name)), name
