"""The smoothed-aggregation surface without a GPU: the two entry points are declared in include/sbhip.h, exported by
libsbhip.so, listed in capi.SYMBOLS and prototyped; the host library exports the aggregation hierarchy builder and the solver
entry, the four drop-in libraries solvePCGMGPolySA with the declared prototype, and the Galerkin entries keep theirs; hostapi
refuses a bad coarsening, theta, omega_s and levels, two ranks, single precision and a host-only problem before the library is
touched, and the default coarsening takes the path of before; the driver's help names -a and its source refuses -a with -g and
without -p mgpoly before the set-up (the run-time refusal needs the device the driver opens first:
tests/test_gpu_aggregation_driver.py)."""
import ctypes
import inspect
import os
import re

import pytest

from test_galerkin_api import Fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")
NEW = {"sb_matrix_aggregate": 5, "sb_matrix_sa_prolongation": 5}


def test_symbols_declared_exported_listed_and_prototyped():
    from sparsebench_amd import capi
    L = capi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbhip.h")).read(), flags=re.S)
    for n, nargs in NEW.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % n, header)
        assert m and len(m.group(1).split(",")) == nargs, "include/sbhip.h does not declare %s with %d arguments" % (n, nargs)
        assert hasattr(L, n) and n in capi.SYMBOLS and len(getattr(L, n).argtypes) == nargs
    assert re.search(r"int\s+sb_matrix_aggregate\s*\(\s*const\s+sb_matrix\s*\*\s*A\s*,\s*double\s+theta\s*,\s*int32_t\s*\*\s*agg_out\s*,"
                     r"\s*uint32_t\s*\*\s*n_agg\s*,\s*uint32_t\s*\*\s*rounds\s*\)\s*;", header)
    assert re.search(r"sb_csr\s*\*\s*sb_matrix_sa_prolongation\s*\(\s*const\s+sb_matrix\s*\*\s*A\s*,\s*double\s+theta\s*,\s*double\s+omega_s\s*,"
                     r"\s*double\s+lmax\s*,\s*uint32_t\s*\*\s*n_agg\s*\)\s*;", header)
    assert L.sb_matrix_sa_prolongation.restype is ctypes.c_void_p and L.sb_matrix_aggregate.restype is ctypes.c_int
    assert len(L.sb_matrix_galerkin.argtypes) == 5 and len(L.sb_pcg_create_mg_poly.argtypes) == 14  # the existing entries keep theirs
    assert L.sb_is_initialized() == 0  # loading touched no device


@pytest.mark.parametrize("lib", ["libsparsebench_crs.so", "libsparsebench_scs.so", "libsparsebench_crs_sp.so", "libsparsebench_scs_sp.so"])
def test_host_and_dropin_libraries_export_the_entries(lib):
    from sparsebench_amd import hostapi
    H = hostapi.host()
    hostapi.host("single")
    for name in ("sbh_mg_hierarchy_build_sa", "sbh_solve_pcg_mgpoly_sa", "sbh_mg_hierarchy_build_galerkin", "sbh_solve_pcg_mgpoly_galerkin"):
        assert hasattr(H, name), name
    d = ctypes.CDLL(os.path.join(LIB, lib))
    assert hasattr(d, "solvePCGMGPolySA") and hasattr(d, "solvePCGMGPolyGalerkin")
    hdr = open(os.path.join(ROOT, "include", "sparsebench", "sparsebench.h")).read()
    assert re.search(r"\bint\s+solvePCGMGPolySA\s*\(\s*Comm\s*\*\s*comm\s*,\s*Parameter\s*\*\s*param\s*,\s*Matrix\s*\*\s*m\s*\)\s*;", hdr)
    m = re.search(r"\bint\s+sbh_solve_pcg_mgpoly_sa\s*\(([^)]*)\)", hdr)
    assert m and len(m.group(1).split(",")) == 10 and re.search(r"int\s+levels\s*,\s*int\s+steps\s*$", m.group(1))
    m = re.search(r"\bvoid\s*\*\s*sbh_mg_hierarchy_build_sa\s*\(([^)]*)\)", hdr)
    assert m and len(m.group(1).split(",")) == 16 and "nx" not in m.group(1)  # no grid
    m = re.search(r"\bvoid\s*\*\s*sbh_mg_hierarchy_build_galerkin\s*\(([^)]*)\)", hdr)
    assert m and len(m.group(1).split(",")) == 11


def test_hostapi_keywords_and_refusals():
    from sparsebench_amd import hostapi
    sig = inspect.signature(hostapi.PCG.__init__).parameters
    assert sig["coarsening"].default == "geometric" and sig["theta"].default is None and sig["omega_s"].default is None
    assert inspect.signature(hostapi.aggregate).parameters["theta"].default == 0.0
    sig = inspect.signature(hostapi.sa_prolongation).parameters
    assert (sig["theta"].default, sig["omega_s"].default, sig["lmax"].default) == (0.0, 4.0 / 3.0, None)
    sig = inspect.signature(hostapi.mg_aggregation).parameters
    assert (sig["levels"].default, sig["theta"].default, sig["omega_s"].default) == (None, 0.0, 4.0 / 3.0)
    file_problem = Fake()
    file_problem.filename = "a.mtx"  # a file is welcome: it gets as far as the library
    file_problem.nr = file_problem.totalNr = 1000  # (more than the coarsest level may have: mg_aggregation has work to do)
    two_ranks, sp, host_only = Fake(), Fake(), Fake()
    two_ranks.totalNr, sp.precision, host_only.upload = 54, "single", False
    for fn in (hostapi.aggregate, hostapi.sa_prolongation, hostapi.mg_aggregation):
        for p, msg in ((two_ranks, "one rank"), (sp, "double precision only"), (host_only, "upload=False")):
            with pytest.raises(ValueError, match=msg):
                fn(p)
        with pytest.raises(AssertionError, match="the library was touched"):
            fn(file_problem)
    for bad in (-0.1, float("nan"), float("inf"), "0", None, True):
        with pytest.raises(ValueError, match="theta must be finite and not negative"):
            hostapi.aggregate(Fake(), bad)
        with pytest.raises(ValueError, match="theta must be finite and not negative"):
            hostapi.sa_prolongation(Fake(), theta=bad)
    for bad in (-1.0, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError, match="omega_s must be finite and not negative"):
            hostapi.sa_prolongation(Fake(), omega_s=bad)
    for bad in (0.0, -2.0, float("inf")):
        with pytest.raises(ValueError, match="lmax must be finite and positive"):
            hostapi.sa_prolongation(Fake(), lmax=bad)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="levels must be 1 or more"):
            hostapi.mg_aggregation(Fake(), levels=bad)
    assert hostapi.mg_aggregation(Fake(), levels=1) == []  # one level: nothing to build, the library is not touched
    assert hostapi.mg_aggregation(Fake()) == []  # 27 rows: the fine level is already the coarsest
    # PCG's keywords
    for bad in ("sa", "Aggregation", None, True):
        with pytest.raises(ValueError, match="coarsening must be 'geometric' or 'aggregation'"):
            hostapi.PCG(Fake(), precond="mgpoly", coarsening=bad)
    for precond in ("jacobi", "sgs", "mg", "mgfw", "poly"):
        with pytest.raises(ValueError, match="coarsening='aggregation' goes with precond='mgpoly' only"):
            hostapi.PCG(Fake(), precond=precond, coarsening="aggregation")
    for kw in (dict(galerkin=True), dict(galerkin="device"), dict(coarse=[])):
        with pytest.raises(ValueError, match="coarsening='aggregation' builds the hierarchy itself"):
            hostapi.PCG(Fake(), precond="mgpoly", coarsening="aggregation", **kw)
    for kw in (dict(theta=0.1), dict(omega_s=1.0), dict(theta=0.0, coarsening="geometric")):
        with pytest.raises(ValueError, match="theta and omega_s go with coarsening='aggregation' only"):
            hostapi.PCG(Fake(), precond="mgpoly", **kw)
    with pytest.raises(ValueError, match="theta must be finite and not negative"):
        hostapi.PCG(Fake(), precond="mgpoly", coarsening="aggregation", theta=-1.0)
    with pytest.raises(TypeError, match="coarsening"):
        hostapi.BiCGStab(Fake(), precond="jacobi", coarsening="aggregation")
    with pytest.raises(ValueError):  # the default is the geometric path: 3 x 3 x 3 has no second level
        hostapi.PCG(Fake(), precond="mgpoly", levels=2)


def test_driver_help_and_messages_name_a():
    import driver_options as opts
    help_text = opts.help_text()
    assert re.search(r"-a\b.*Smoothed-aggregation coarsening.*-p mgpoly.*any matrix", help_text)
    assert re.search(r"-g\b.*Galerkin coarse operators.*-p mgpoly", help_text) and "-C <int>" in help_text  # the help text is still whole
    size, MGPOLY, A = opts.SIZE, opts.KIND["mgpoly"], opts.COARSE["aggregation"]
    # -a is a switch of its own, takes no argument, and lands in the spec's coarse operators: at the defaults (solvePCGMGPolySA's
    # spec; the symbol itself runs in test_gpu_aggregation_driver.py) and beside -l and -d, by -p and by -P
    for head, byP in ((["-t", "pcg", "-p"], 0), (["-t", "bicgstab", "-P"], 1), (["-t", "gmres", "-P"], 1)):
        for extra, levels, steps in (([], 0, 0), (["-l", "3"], 3, 0), (["-d", "1"], 0, 1), (["-l", "2", "-d", "4"], 2, 4)):
            p = opts.accepted(head + ["mgpoly", "-a"] + extra + size)
            assert p.spec == (MGPOLY, levels, steps, A) and p.byP == byP and p.type == opts.TYPE[head[1]]
    # the existing paths
    assert opts.accepted(["-t", "pcg", "-p", "mgpoly", "-g"] + size).spec == (MGPOLY, 0, 0, opts.COARSE["galerkin"])
    assert opts.accepted(["-t", "pcg", "-p", "mgpoly"] + size).spec == (MGPOLY, 0, 0, opts.COARSE["regenerated"])
    for args, msg in ((["-t", "pcg", "-p", "mgpoly", "-a", "-g"], "it does not go with -g"),
                      (["-t", "bicgstab", "-P", "mgpoly", "-g", "-a"], "it does not go with -g"),
                      (["-t", "pcg", "-p", "mgfw", "-a"], "-a (smoothed-aggregation coarsening) goes with -p mgpoly only"),
                      (["-t", "pcg", "-a"], "-a (smoothed-aggregation coarsening) goes with -p mgpoly only"),
                      (["-a"], "-a (smoothed-aggregation coarsening) goes with -p mgpoly only")):
        opts.refused(args + ["-i", "10"] + size, msg)
    # a file has no grid, and -a asks for none: any matrix, and levels that no grid rule bounds
    for head in (["-t", "pcg", "-p"], ["-t", "bicgstab", "-P"], ["-t", "gmres", "-P"]):
        opts.refused(head + ["mgpoly", "-m", "a.mtx"], "-%s mgpoly needs the grid: its hierarchy is the generated matrix's on coarser grids, not -m a.mtx\n"
                     % head[2][1])
        p = opts.accepted(head + ["mgpoly", "-a", "-m", "a.mtx"])
        assert p.spec == (MGPOLY, 0, 0, A) and p.filename == "a.mtx"
    for kind in ("mg", "mgfw"):
        opts.refused(["-t", "pcg", "-p", kind, "-m", "a.mtx"], "-p %s needs the grid" % kind)
    opts.refused(["-t", "pcg", "-p", "mgpoly", "-l", "6"] + size, "6 levels")
    assert opts.accepted(["-t", "pcg", "-p", "mgpoly", "-a", "-l", "6"] + size).spec == (MGPOLY, 6, 0, A)
    opts.refused(["-t", "pcg", "-p", "mgpoly", "-a", "-i", "10"] + size, "PCG: double precision only", precision="single")
    assert opts.no_device_was_touched()  # before the set-up: the parser has no way to a device
