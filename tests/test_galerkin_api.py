"""The device Galerkin product's surface without a GPU: the new entry points are declared in include/sbhip.h,
exported by libsbhip.so, listed in capi.SYMBOLS and prototyped; the host library exports the Galerkin hierarchy builder, the solver
entry and the in-memory Problem, the four drop-in libraries solvePCGMGPolyGalerkin with the declared prototype, and the existing
entries keep theirs; hostapi refuses bad `product` and `galerkin` values, galerkin="device" with coarse=, a file problem, two
ranks and single precision before the library is touched; the driver's help names -g and its source refuses -g without -p mgpoly
before the set-up (the run-time refusal needs the device the driver opens first: tests/test_gpu_galerkin_driver.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")

NEW = {"sb_matrix_galerkin": 5, "sb_csr_rows": 1, "sb_csr_nnz": 1, "sb_csr_copy": 4, "sb_csr_stats": 2, "sb_csr_free": 1}


def test_galerkin_symbols_declared_exported_listed_and_prototyped():
    from sparsebench_amd import capi
    L = capi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbhip.h")).read(), flags=re.S)
    assert re.search(r"typedef\s+struct\s+sb_csr\s+sb_csr\s*;", header)
    for n, nargs in NEW.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % n, header)
        assert m, "include/sbhip.h does not declare %s" % n
        assert len(m.group(1).split(",")) == nargs, "include/sbhip.h declares %s with other arguments" % n
        assert hasattr(L, n), "libsbhip.so does not export %s" % n
        assert n in capi.SYMBOLS
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == nargs, "capi.load() prototypes %s wrongly" % n
    assert re.search(r"sb_csr\s*\*\s*sb_matrix_galerkin\s*\(\s*const\s+sb_matrix\s*\*\s*A\s*,\s*uint32_t\s+nCoarse\s*,\s*const\s+uint64_t\s*\*\s*p_ptr\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*p_col\s*,\s*const\s+double\s*\*\s*p_val\s*\)\s*;", header)
    assert L.sb_matrix_galerkin.restype is ctypes.c_void_p and L.sb_csr_nnz.restype is ctypes.c_uint64 and L.sb_csr_rows.restype is ctypes.c_uint32
    assert len(L.sb_pcg_create_mg_poly.argtypes) == 14 and len(L.sb_pcg_create_mg_p.argtypes) == 10  # the existing kinds keep theirs
    assert L.sb_is_initialized() == 0  # loading touched no device


@pytest.mark.parametrize("lib", ["libsparsebench_crs.so", "libsparsebench_scs.so", "libsparsebench_crs_sp.so", "libsparsebench_scs_sp.so"])
def test_host_and_dropin_libraries_export_the_galerkin_entries(lib):
    from sparsebench_amd import hostapi
    H = hostapi.host()
    hostapi.host("single")
    for name in ("sbh_mg_hierarchy_build_galerkin", "sbh_solve_pcg_mgpoly_galerkin", "sbh_problem_create_csr", "sbh_gmatrix_from_csr",
                 "sbh_mg_hierarchy_build", "sbh_solve_pcg_mgpoly"):
        assert hasattr(H, name), name
    d = ctypes.CDLL(os.path.join(LIB, lib))
    assert hasattr(d, "solvePCGMGPolyGalerkin") and hasattr(d, "solvePCGMGPoly")
    hdr = open(os.path.join(ROOT, "include", "sparsebench", "sparsebench.h")).read()
    assert re.search(r"\bint\s+solvePCGMGPolyGalerkin\s*\(\s*Comm\s*\*\s*comm\s*,\s*Parameter\s*\*\s*param\s*,\s*Matrix\s*\*\s*m\s*\)\s*;", hdr)
    m = re.search(r"\bint\s+sbh_solve_pcg_mgpoly_galerkin\s*\(([^)]*)\)", hdr)
    assert m and len(m.group(1).split(",")) == 10 and re.search(r"int\s+levels\s*,\s*int\s+steps\s*$", m.group(1))
    # the existing entries keep their prototypes
    m = re.search(r"\bint\s+sbh_solve_pcg_mgpoly\s*\(([^)]*)\)", hdr)
    assert m and len(m.group(1).split(",")) == 10
    m = re.search(r"\bvoid\s*\*\s*sbh_mg_hierarchy_build\s*\(([^)]*)\)", hdr)
    assert m and len(m.group(1).split(",")) == 7
    m = re.search(r"\bvoid\s*\*\s*sbh_mg_hierarchy_build_galerkin\s*\(([^)]*)\)", hdr)
    assert m and len(m.group(1).split(",")) == 11


class Fake:
    precision, filename, nr, totalNr, dims, upload = "double", "generate", 27, 27, (3, 3, 3), True

    def rhs(self):
        raise AssertionError("the library was touched")

    matrix = property(lambda self: (_ for _ in ()).throw(AssertionError("the library was touched")))


def test_hostapi_keywords_and_refusals():
    from sparsebench_amd import hostapi
    import inspect
    assert inspect.signature(hostapi.mg_galerkin).parameters["product"].default == "scipy"
    assert list(inspect.signature(hostapi.mg_galerkin).parameters)[:4] == ["problem", "levels", "directory", "_owned"]
    assert callable(hostapi.galerkin_product) and callable(hostapi.Problem.from_csr)
    for bad in ("gpu", "Device", None, True):
        with pytest.raises(ValueError, match="product must be 'scipy' or 'device'"):
            hostapi.mg_galerkin(Fake(), product=bad)
    with pytest.raises(ValueError, match="takes no directory"):
        hostapi.mg_galerkin(Fake(), directory="/nowhere", product="device")
    file_problem = Fake()
    file_problem.filename = "a.mtx"
    two_ranks = Fake()
    two_ranks.totalNr = 54
    sp = Fake()
    sp.precision = "single"
    host_only = Fake()
    host_only.upload = False
    for p, msg in ((file_problem, "mg_galerkin needs the grid"), (two_ranks, "one rank"), (sp, "double precision only"),
                   (host_only, "upload=False")):
        with pytest.raises(ValueError, match=msg):
            hostapi.mg_galerkin(p, product="device")
        if p is not host_only:
            with pytest.raises(ValueError, match=msg):
                hostapi.PCG(p, precond="mgpoly", galerkin="device")
    with pytest.raises(ValueError):  # 3 x 3 x 3 has no second level
        hostapi.mg_galerkin(Fake(), levels=2, product="device")
    P = (np.zeros(28, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0))
    for p, msg in ((two_ranks, "galerkin_product runs on one rank"), (sp, "galerkin_product: double precision only"),
                   (host_only, "galerkin_product reads the uploaded matrix")):
        with pytest.raises(ValueError, match=msg):
            hostapi.galerkin_product(p, P)
    with pytest.raises(ValueError, match="P of level 0 must have 28 row pointers"):
        hostapi.galerkin_product(Fake(), (np.zeros(5, dtype=np.uint64), P[1], P[2]))
    # PCG's galerkin keyword: True, False or "device"
    for bad in (1, 0, "scipy", "Device", None):
        with pytest.raises(ValueError, match="galerkin must be True or False"):
            hostapi.PCG(Fake(), precond="mgpoly", galerkin=bad)
    with pytest.raises(ValueError, match="galerkin='device' builds the coarse operators itself"):
        hostapi.PCG(Fake(), precond="mgpoly", galerkin="device", coarse=[])
    with pytest.raises(ValueError, match="galerkin=True builds the coarse operators itself"):
        hostapi.PCG(Fake(), precond="mgpoly", galerkin=True, coarse=[])
    for precond in ("jacobi", "sgs", "mg", "mgfw", "poly"):
        with pytest.raises(ValueError, match="coarse_steps and galerkin go with precond='mgpoly' only"):
            hostapi.PCG(Fake(), precond=precond, galerkin="device")
    with pytest.raises(ValueError):  # 3 x 3 x 3 has no second level: refused before the library is touched
        hostapi.PCG(Fake(), precond="mgpoly", galerkin="device", levels=2)


def test_driver_help_and_messages_name_g():
    import driver_options as opts
    help_text = opts.help_text()
    assert re.search(r"-g\b.*Galerkin coarse operators.*-p mgpoly", help_text)
    assert re.search(r"-p <jacobi\|sgs>.*Default jacobi", help_text) and "-C <int>" in help_text  # the help text is still whole
    SIZE, MGPOLY, G = opts.SIZE + ["-i", "10"], opts.KIND["mgpoly"], opts.COARSE["galerkin"]
    # -g is a switch of its own, takes no argument, and lands in the spec's coarse operators: at the defaults
    # (solvePCGMGPolyGalerkin's spec; the symbol itself runs in test_gpu_galerkin_driver.py) and beside -l and -d, by -p and by -P
    for head, byP in ((["-t", "pcg", "-p"], 0), (["-t", "bicgstab", "-P"], 1), (["-t", "gmres", "-P"], 1)):
        for extra, levels, steps in (([], 0, 0), (["-l", "3"], 3, 0), (["-d", "1"], 0, 1), (["-l", "2", "-d", "4"], 2, 4)):
            p = opts.accepted(head + ["mgpoly", "-g"] + extra + SIZE)
            assert p.spec == (MGPOLY, levels, steps, G) and p.byP == byP and p.type == opts.TYPE[head[1]] and p.dims == (16, 16, 16)
            assert opts.accepted(head + ["mgpoly"] + extra + SIZE).spec == (MGPOLY, levels, steps, 0)  # without it: the path of before
    for args in (["-t", "pcg", "-p", "mgfw", "-g"], ["-t", "pcg", "-g"], ["-g"], ["-t", "pcg", "-p", "poly", "-g"]):
        opts.refused(args + SIZE, "-g (Galerkin coarse operators) goes with -p mgpoly only\n")  # status 1, on stderr
    opts.refused(["-t", "pcg", "-p", "mgpoly", "-g"] + SIZE, "PCG: double precision only", precision="single")
    assert opts.no_device_was_touched()  # before the set-up: the parser has no way to a device
