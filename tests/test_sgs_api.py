"""The SGS surface without a GPU: the new entry points are declared in include/sbhip.h, exported by libsbhip.so,
listed in capi.SYMBOLS and prototyped, and sb_pcg_create keeps its five arguments; the four drop-in libraries export
solvePCGSGS with the declared prototype; hostapi.PCG refuses a single-precision problem and bad precond / dinv combinations
before it touches the library; the driver's help names -p; loading initialises no device."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")

NEW = {"sb_pcg_create_sgs": 4, "sb_pcg_precond": 1, "sb_pcg_colours": 1, "sb_pcg_colouring": 2, "sb_pcg_apply_precond": 3,
       "sb_pcg_precond_bytes": 1, "sb_pcg_apply_precond_ms": 2}


def test_sgs_symbols_declared_exported_listed_and_prototyped():
    from sparsebench_amd import capi
    L = capi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbhip.h")).read(), flags=re.S)
    for n, nargs in NEW.items():
        assert re.search(r"\b%s\s*\(" % n, header), "include/sbhip.h does not declare %s" % n
        assert hasattr(L, n), "libsbhip.so does not export %s" % n
        assert n in capi.SYMBOLS
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == nargs, "capi.load() prototypes %s wrongly" % n
    assert L.sb_pcg_precond_bytes.restype is ctypes.c_double and L.sb_pcg_colours.restype is ctypes.c_int
    assert len(L.sb_pcg_create.argtypes) == 5
    m = re.search(r"\bsb_pcg_create\s*\(([^)]*)\)", header)
    assert m and len(m.group(1).split(",")) == 5
    assert L.sb_is_initialized() == 0  # loading touched no device


@pytest.mark.parametrize("lib", ["libsparsebench_crs.so", "libsparsebench_scs.so", "libsparsebench_crs_sp.so", "libsparsebench_scs_sp.so"])
def test_dropin_libraries_export_solvePCGSGS(lib):
    from sparsebench_amd import hostapi
    hostapi.host()
    hostapi.host("single")
    d = ctypes.CDLL(os.path.join(LIB, lib))
    assert hasattr(d, "solvePCGSGS") and hasattr(d, "solvePCG")
    hdr = open(os.path.join(ROOT, "include", "sparsebench", "sparsebench.h")).read()
    assert re.search(r"\bint\s+solvePCGSGS\s*\(\s*Comm\s*\*\s*comm\s*,\s*Parameter\s*\*\s*param\s*,\s*Matrix\s*\*\s*m\s*\)\s*;", hdr)


def test_hostapi_pcg_refuses_before_the_library_is_touched():
    from sparsebench_amd import hostapi

    class Fake:  # never touched: the refusal comes first
        precision = "double"
        nr = 4

        def rhs(self):
            raise AssertionError("the library was touched")

    class FakeSP(Fake):
        precision = "single"

    for precond in ("jacobi", "sgs"):
        with pytest.raises(ValueError, match="double precision only"):
            hostapi.PCG(FakeSP(), precond=precond)
    with pytest.raises(ValueError, match="takes no dinv"):
        hostapi.PCG(Fake(), np.ones(4), precond="sgs")
    with pytest.raises(ValueError, match="takes no dinv"):
        hostapi.PCG(Fake(), dinv=np.ones(4), precond="sgs")
    for bad in ("ilu", "SGS", None, ""):
        with pytest.raises(ValueError, match="precond must be 'jacobi' or 'sgs'"):
            hostapi.PCG(Fake(), precond=bad)
    for name in ("precond", "colours", "colouring", "apply", "precond_bytes", "solve", "start", "run_iters", "finish", "history",
                 "solution", "dinv", "launches_per_body", "counters", "free"):
        assert callable(getattr(hostapi.PCG, name)), name


def test_driver_help_names_the_preconditioner_switch():
    import driver_options as opts
    help_text = opts.help_text()
    assert re.search(r"-p <jacobi\|sgs>.*Default jacobi", help_text)
    assert re.search(r"-t <bench type>.*\bpcg\b", help_text) and "-C <int>" in help_text  # the help text is still whole
    small = ["-x", "8", "-y", "8", "-z", "8", "-i", "10"]
    for name in ("sgs", "jacobi"):
        p = opts.accepted(["-t", "pcg", "-p", name] + small)
        assert p.type == opts.TYPE["pcg"] and p.spec == (opts.KIND[name], 0, 0, 0) and not p.byP
    for t in ("cg", "gmres", "spmv", "bicgstab"):
        opts.refused(["-t", t, "-p", "sgs"] + small, "goes with -t pcg only")
    opts.refused(["-p", "sgs"] + small, "goes with -t pcg only")  # the default type is cg
    opts.refused(["-t", "pcg", "-p", "ilu"] + small, "Unknown preconditioner ilu")
    opts.refused(["-t", "pcg", "-p", "sgs"] + small, "PCG: double precision only", precision="single")
    opts.refused(["-t", "cheb"] + small, "Unknown solver type cheb\n", stream="stdout")  # still an unknown type
    assert opts.no_device_was_touched()
