"""The MG surface without a GPU: the new entry points are declared in include/sbhip.h, exported by libsbhip.so,
listed in capi.SYMBOLS and prototyped; the four drop-in libraries export solvePCGMG with the declared prototype; hostapi.PCG
refuses a single-precision problem and bad precond / dinv / levels / coarse combinations before it touches the library; the
driver's help names -p mg and -l."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")

NEW = {"sb_pcg_create_mg": 7, "sb_pcg_levels": 1, "sb_pcg_level_rows": 2, "sb_pcg_level_colours": 2}


def test_mg_symbols_declared_exported_listed_and_prototyped():
    from sparsebench_amd import capi
    L = capi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbhip.h")).read(), flags=re.S)
    for n, nargs in NEW.items():
        assert re.search(r"\b%s\s*\(" % n, header), "include/sbhip.h does not declare %s" % n
        assert hasattr(L, n), "libsbhip.so does not export %s" % n
        assert n in capi.SYMBOLS
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == nargs, "capi.load() prototypes %s wrongly" % n
    assert L.sb_pcg_levels.restype is ctypes.c_int and L.sb_pcg_level_rows.restype is ctypes.c_uint32
    m = re.search(r"\bsb_pcg_create_mg\s*\(([^)]*)\)", header)
    assert m and len(m.group(1).split(",")) == 7
    assert len(L.sb_pcg_create_sgs.argtypes) == 4 and len(L.sb_pcg_create.argtypes) == 5  # as they were


@pytest.mark.parametrize("lib", ["libsparsebench_crs.so", "libsparsebench_scs.so", "libsparsebench_crs_sp.so", "libsparsebench_scs_sp.so"])
def test_dropin_libraries_export_solvePCGMG(lib):
    from sparsebench_amd import hostapi
    hostapi.host()
    hostapi.host("single")
    d = ctypes.CDLL(os.path.join(LIB, lib))
    assert hasattr(d, "solvePCGMG") and hasattr(d, "solvePCGSGS") and hasattr(d, "solvePCG")
    hdr = open(os.path.join(ROOT, "include", "sparsebench", "sparsebench.h")).read()
    assert re.search(r"\bint\s+solvePCGMG\s*\(\s*Comm\s*\*\s*comm\s*,\s*Parameter\s*\*\s*param\s*,\s*Matrix\s*\*\s*m\s*\)\s*;", hdr)


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
        hostapi.PCG(FakeSP(), precond="mg")
    with pytest.raises(ValueError, match="double precision only"):
        hostapi.PCG(FakeSP(), precond="mg", levels=2)
    for bad in ("ilu", "MG", "amg", None, ""):
        with pytest.raises(ValueError, match="precond must be 'jacobi' or 'sgs' or 'mg'"):
            hostapi.PCG(Fake(), precond=bad)
    with pytest.raises(ValueError, match="takes no dinv"):
        hostapi.PCG(Fake(), np.ones(4), precond="mg")
    with pytest.raises(ValueError, match="takes no dinv"):
        hostapi.PCG(Fake(), dinv=np.ones(4), precond="mg", levels=2)
    with pytest.raises(ValueError, match="not both"):
        hostapi.PCG(Fake(), precond="mg", levels=2, coarse=[(Fake(), np.arange(4))])
    for precond in ("jacobi", "sgs"):
        with pytest.raises(ValueError, match="go with precond='mg' only"):
            hostapi.PCG(Fake(), precond=precond, levels=2)
        with pytest.raises(ValueError, match="go with precond='mg' only"):
            hostapi.PCG(Fake(), precond=precond, coarse=[])
    with pytest.raises(ValueError, match="needs the grid"):  # a problem that was not generated and brings no hierarchy
        hostapi.PCG(Fake(), precond="mg")
    for name in ("levels", "level_rows", "level_colours", "precond", "colours", "colouring", "apply", "precond_bytes", "solve",
                 "launches_per_body", "free"):
        assert callable(getattr(hostapi.PCG, name)), name


def test_driver_help_names_mg_and_its_levels():
    import driver_options as opts
    help_text = opts.help_text()
    assert re.search(r"-p mg\b", help_text) and re.search(r"-l <int>", help_text)
    assert re.search(r"-p <jacobi\|sgs>.*Default jacobi", help_text) and "-C <int>" in help_text  # the help text is still whole
    small, SIZE = ["-i", "10"], opts.SIZE
    assert opts.accepted(["-t", "pcg", "-p", "mg"] + small + SIZE).spec == (opts.KIND["mg"], 0, 0, 0)
    p = opts.accepted(["-t", "pcg", "-p", "mg", "-l", "3"] + small + SIZE)  # the path that is not the drop-in symbol's defaults
    assert p.type == opts.TYPE["pcg"] and p.spec == (opts.KIND["mg"], 3, 0, 0) and not p.byP
    opts.refused(["-t", "pcg", "-p", "mg", "-m", "tri.mtx"] + small, "needs the grid")
    for extra in ([], ["-p", "sgs"], ["-p", "jacobi"]):
        opts.refused(["-t", "pcg", "-l", "2"] + extra + small + SIZE, "goes with -p mg only")
    opts.refused(["-t", "pcg", "-p", "mg", "-l", "5"] + small + SIZE, "5 levels would give a coarse dimension smaller than 2")
    opts.refused(["-t", "pcg", "-p", "mg", "-l", "2", "-x", "15", "-y", "16", "-z", "16"] + small, "2 levels need every dimension divisible by 2")
    opts.refused(["-t", "cg", "-p", "mg"] + small + SIZE, "goes with -t pcg only")
    opts.refused(["-t", "pcg", "-p", "amg"] + small + SIZE, "Unknown preconditioner amg (-p <jacobi|sgs>)\n")
    opts.refused(["-t", "pcg", "-p", "mg"] + small + SIZE, "PCG: double precision only", precision="single")
    assert opts.no_device_was_touched()
