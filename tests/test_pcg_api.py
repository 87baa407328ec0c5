"""The PCG surface without a GPU: the new entry points are declared in include/sbhip.h, exported by libsbhip.so, listed in
capi.SYMBOLS and prototyped; the four drop-in libraries export solvePCG with the declared prototype; hostapi.PCG refuses a
single-precision problem before it touches the library; the driver's help names the type; loading initialises no device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")

NEW = ["sb_matrix_diagonal", "sb_pcg_create", "sb_pcg_free", "sb_pcg_solve", "sb_pcg_start", "sb_pcg_run_iters", "sb_pcg_finish",
       "sb_pcg_history", "sb_pcg_solution", "sb_pcg_check_residual", "sb_pcg_dinv", "sb_pcg_launches_per_body", "sb_pcg_loop_ms",
       "sb_pcg_counters", "sb_pcg_update_r_native", "sb_pcg_update_r_launch"]


def test_pcg_symbols_declared_exported_listed_and_prototyped():
    from sparsebench_amd import capi
    L = capi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbhip.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), "include/sbhip.h does not declare %s" % n
        assert hasattr(L, n), "libsbhip.so does not export %s" % n
        assert n in capi.SYMBOLS
        assert getattr(L, n).argtypes is not None, "capi.load() gives %s no prototype" % n
    assert len(L.sb_pcg_create.argtypes) == 5 and len(L.sb_pcg_history.argtypes) == 8 and len(L.sb_pcg_update_r_native.argtypes) == 8
    assert L.sb_is_initialized() == 0  # loading touched no device


@pytest.mark.parametrize("lib", ["libsparsebench_crs.so", "libsparsebench_scs.so", "libsparsebench_crs_sp.so", "libsparsebench_scs_sp.so"])
def test_dropin_libraries_export_solvePCG(lib):
    from sparsebench_amd import hostapi
    hostapi.host()
    hostapi.host("single")
    d = ctypes.CDLL(os.path.join(LIB, lib))
    assert hasattr(d, "solvePCG")
    hdr = open(os.path.join(ROOT, "include", "sparsebench", "sparsebench.h")).read()
    assert re.search(r"\bint\s+solvePCG\s*\(\s*Comm\s*\*\s*comm\s*,\s*Parameter\s*\*\s*param\s*,\s*Matrix\s*\*\s*m\s*\)\s*;", hdr)


def test_hostapi_pcg_refuses_single_precision_and_has_its_methods():
    from sparsebench_amd import hostapi

    class FakeSP:  # never touched: the refusal comes first
        precision = "single"

        def rhs(self):
            raise AssertionError("the library was touched")

    with pytest.raises(ValueError, match="double precision only"):
        hostapi.PCG(FakeSP())
    for name in ("solve", "start", "run_iters", "finish", "history", "solution", "check_residual", "dinv", "launches_per_body",
                 "loop_ms", "counters", "free"):
        assert callable(getattr(hostapi.PCG, name)), name


def test_driver_help_names_pcg_and_the_sp_drivers_refuse_it():
    src = open(os.path.join(ROOT, "sparsebench_amd", "host", "sbh_main.c")).read()
    help_text = "".join(re.findall(r'^\s+"(.*)"\s*;?\s*$', src.split("kHelp =")[1].split(";")[0], flags=re.M))
    assert re.search(r"-t <bench type>.*\bpcg\b", help_text)
    assert 'strcmp(optarg, "pcg") == 0' in src and "PCG: double precision only" in src
    assert 'strcmp(optarg, "cheb")' not in src  # still an unknown type
