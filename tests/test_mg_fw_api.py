"""The surface of the V-cycle with full-weighting transfers without a GPU: the new entry points are declared in
include/sbhip.h, exported by libsbhip.so, listed in capi.SYMBOLS and prototyped; the four drop-in libraries export solvePCGMGFW
with the declared prototype; hostapi.PCG refuses bad precond / levels / coarse / P / omega combinations before it touches the
library; the library's own refusals are worded, each naming the level; the driver's help names -p mgfw."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")

NEW = {"sb_pcg_create_mg_p": 10, "sb_pcg_mg_fw_probe": 8}


def test_symbols_declared_exported_listed_and_prototyped():
    from sparsebench_amd import capi
    L = capi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbhip.h")).read(), flags=re.S)
    for n, nargs in NEW.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % n, header)
        assert m and len(m.group(1).split(",")) == nargs, "include/sbhip.h does not declare %s with %d arguments" % (n, nargs)
        assert hasattr(L, n), "libsbhip.so does not export %s" % n
        assert n in capi.SYMBOLS
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == nargs, "capi.load() prototypes %s wrongly" % n
    assert L.sb_pcg_create_mg_p.restype is ctypes.c_void_p and L.sb_pcg_mg_fw_probe.restype is None
    assert len(L.sb_pcg_create_mg.argtypes) == 7 and len(L.sb_pcg_create_sgs.argtypes) == 4  # as they were
    assert "3 MG with full-weighting transfers" in open(os.path.join(ROOT, "include", "sbhip.h")).read()


@pytest.mark.parametrize("lib", ["libsparsebench_crs.so", "libsparsebench_scs.so", "libsparsebench_crs_sp.so", "libsparsebench_scs_sp.so"])
def test_dropin_libraries_export_solvePCGMGFW(lib):
    from sparsebench_amd import hostapi
    hostapi.host()
    hostapi.host("single")
    d = ctypes.CDLL(os.path.join(LIB, lib))
    assert hasattr(d, "solvePCGMGFW") and hasattr(d, "solvePCGMG") and hasattr(d, "solvePCGSGS")
    hdr = open(os.path.join(ROOT, "include", "sparsebench", "sparsebench.h")).read()
    assert re.search(r"\bint\s+solvePCGMGFW\s*\(\s*Comm\s*\*\s*comm\s*,\s*Parameter\s*\*\s*param\s*,\s*Matrix\s*\*\s*m\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+sbh_solve_pcg_mgfw\s*\(", hdr) and re.search(r"\bvoid\s+sbh_mg_trilinear\s*\(", hdr)
    assert hasattr(hostapi.host(), "sbh_solve_pcg_mgfw") and hasattr(hostapi.host(), "sbh_mg_trilinear")


def test_hostapi_pcg_refuses_before_the_library_is_touched():
    from sparsebench_amd import hostapi

    class Fake:  # never touched: the refusal comes first
        precision = "double"
        nr = 4

        def rhs(self):
            raise AssertionError("the library was touched")

    class Small(Fake):
        nr = 2

    class FakeSP(Fake):
        precision = "single"

    P = (np.array([0, 1, 2, 3, 4]), np.array([0, 0, 1, 1]), np.ones(4))
    with pytest.raises(ValueError, match="double precision only"):
        hostapi.PCG(FakeSP(), precond="mgfw")
    with pytest.raises(ValueError, match="double precision only"):
        hostapi.PCG(Fake(), precond="mgfw", coarse=[(FakeSP(), P, 0.5)])
    with pytest.raises(ValueError, match="precond must be 'jacobi' or 'sgs' or 'mg' or 'mgfw'"):
        hostapi.PCG(Fake(), precond="fw")
    with pytest.raises(ValueError, match="takes no dinv"):
        hostapi.PCG(Fake(), np.ones(4), precond="mgfw")
    with pytest.raises(ValueError, match="not both"):
        hostapi.PCG(Fake(), precond="mgfw", levels=2, coarse=[(Small(), P, 0.5)])
    with pytest.raises(ValueError, match="precond='mgfw' needs the grid"):  # not generated and brings no hierarchy
        hostapi.PCG(Fake(), precond="mgfw")
    with pytest.raises(ValueError, match=r"takes coarse=\[\(Problem, P, omega\), \.\.\.\]: entry 0"):
        hostapi.PCG(Fake(), precond="mgfw", coarse=[(Small(), np.arange(2))])  # an injection map is not a transfer
    for omega in (0.0, -0.5, float("nan"), float("inf"), None, "0.5"):
        with pytest.raises(ValueError, match="omega of level 0 must be finite and positive"):
            hostapi.PCG(Fake(), precond="mgfw", coarse=[(Small(), P, omega)])
    with pytest.raises(ValueError, match="P of level 0 must have 5 row pointers"):
        hostapi.PCG(Fake(), precond="mgfw", coarse=[(Small(), (P[0][:4], P[1], P[2]), 0.5)])
    with pytest.raises(ValueError, match="P of level 0: 4 columns, 3 weights"):
        hostapi.PCG(Fake(), precond="mgfw", coarse=[(Small(), (P[0], P[1], P[2][:3]), 0.5)])
    with pytest.raises(ValueError, match="row pointers up to 9"):
        hostapi.PCG(Fake(), precond="mgfw", coarse=[(Small(), (np.array([0, 1, 2, 3, 9]), P[1], P[2]), 0.5)])
    with pytest.raises(ValueError, match="negative pointer or column"):
        hostapi.PCG(Fake(), precond="mgfw", coarse=[(Small(), (P[0], np.array([0, -1, 1, 1]), P[2]), 0.5)])
    with pytest.raises(ValueError, match="scipy.sparse matrix or a \\(ptr, col, val\\) triple"):
        hostapi.PCG(Fake(), precond="mgfw", coarse=[(Small(), 7, 0.5)])
    sp = pytest.importorskip("scipy.sparse")
    with pytest.raises(ValueError, match=r"P of level 0 must be 4 x 2, got \(4, 3\)"):
        hostapi.PCG(Fake(), precond="mgfw", coarse=[(Small(), sp.csr_matrix((P[2], P[1], P[0]), shape=(4, 3)), 0.5)])
    with pytest.raises(AssertionError, match="the library was touched"):  # a sound hierarchy gets as far as the library
        hostapi.PCG(Fake(), precond="mgfw", coarse=[(Small(), sp.csr_matrix((P[2], P[1], P[0]), shape=(4, 2)), 0.5)])
    for name in ("mg_fw_probe", "levels", "level_rows", "precond", "apply", "precond_bytes", "launches_per_body"):
        assert callable(getattr(hostapi.PCG, name)), name


def test_mg_trilinear_refuses_odd_grids():
    from sparsebench_amd import hostapi
    for dims in ((5, 8, 8), (8, 8, 3), (0, 2, 2)):
        with pytest.raises(ValueError, match="odd or empty dimension"):
            hostapi.mg_trilinear(*dims)
    ptr, col, val = hostapi.mg_trilinear(2, 2, 2)  # one coarse point: every fine point takes it, the odd ones with their half weights
    assert ptr.tolist() == list(range(9)) and col.tolist() == [0] * 8 and val.tolist() == [1.0, 0.5, 0.5, 0.25, 0.5, 0.25, 0.25, 0.125]


def test_the_librarys_refusals_name_the_level():
    src = open(os.path.join(ROOT, "sparsebench_amd", "csrc", "sbhip_mg_fw.inc.h")).read()
    for msg in ("omega[%d] = %g: the restriction's scale of level %d must be finite and positive",
                "level %d: the prolongation's row pointer falls from", "outside the %u rows of level %d",
                "level %d: the prolongation's row %u has a weight that is not finite",
                "sb_pcg_mg_fw_probe between sb_pcg_start and sb_pcg_finish"):
        assert msg in src, msg


def test_driver_help_names_mgfw():
    import driver_options as opts
    help_text = opts.help_text()
    assert re.search(r"-p mgfw\b", help_text) and re.search(r"-p mg\b", help_text) and re.search(r"-l <int>", help_text)
    small, SIZE = ["-i", "10"], opts.SIZE
    # the defaults are solvePCGMGFW's spec (the symbol itself runs in test_gpu_mg_fw_driver.py); -l is the other path
    assert opts.accepted(["-t", "pcg", "-p", "mgfw"] + small + SIZE).spec == (opts.KIND["mgfw"], 0, 0, 0)
    assert opts.accepted(["-t", "pcg", "-p", "mgfw", "-l", "3"] + small + SIZE).spec == (opts.KIND["mgfw"], 3, 0, 0)
    opts.refused(["-t", "pcg", "-p", "mgfw", "-m", "tri.mtx"] + small, "-p mgfw needs the grid")
    opts.refused(["-t", "pcg", "-p", "mgfw", "-l", "5"] + small + SIZE, "5 levels would give a coarse dimension smaller than 2")
    opts.refused(["-t", "pcg", "-p", "mgfw", "-l", "2", "-x", "15", "-y", "16", "-z", "16"] + small, "2 levels need every dimension divisible by 2")
    opts.refused(["-t", "cg", "-p", "mgfw"] + small + SIZE, "goes with -t pcg only")
    opts.refused(["-t", "pcg", "-p", "mgfx"] + small + SIZE, "Unknown preconditioner mgfx")
    opts.refused(["-t", "pcg", "-p", "mgfw"] + small + SIZE, "PCG: double precision only", precision="single")
    assert opts.no_device_was_touched()
