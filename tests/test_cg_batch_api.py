"""The batched-CG surface without a GPU: the new entry points are declared in include/sbhip.h, exported by libsbhip.so and
listed in capi.SYMBOLS; the four drop-in libraries export solveCGBatch; hostapi.BatchCG refuses a single-precision problem
before it touches the library; loading initialises no device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")

NEW = ["sb_spmmv_native", "sb_spmmv_native_dot", "sb_block_interleave", "sb_block_deinterleave", "sb_matrix_spmmv_bytes",
       "sb_cgb_create", "sb_cgb_free", "sb_cgb_nrhs", "sb_cgb_launches_per_body", "sb_cgb_solve", "sb_cgb_start", "sb_cgb_run_iters",
       "sb_cgb_finish", "sb_cgb_iterations", "sb_cgb_history", "sb_cgb_solution", "sb_cgb_check_residual", "sb_cgb_loop_ms",
       "sb_cgb_counters",
       # the blocking test entries of the loop's vector kernels and the launch queries (tests/test_gpu_batch_vec_kernels.py,
       # tests/test_gpu_gmres_kernels.py)
       "sb_block_vec_native", "sb_block_vec_launch", "sb_cgb_update_p_native", "sb_cgb_x_finalize_native", "sb_cgb_rows_launch",
       "sb_gmres_group_launch"]
ARGS = {"sb_block_vec_native": 9, "sb_block_vec_launch": 2, "sb_cgb_update_p_native": 10, "sb_cgb_x_finalize_native": 6,
        "sb_cgb_rows_launch": 2, "sb_gmres_group_launch": 2}


def test_batch_symbols_declared_exported_and_listed():
    from sparsebench_amd import capi
    L = capi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbhip.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), "include/sbhip.h does not declare %s" % n
        assert hasattr(L, n), "libsbhip.so does not export %s" % n
        assert n in capi.SYMBOLS
        assert getattr(L, n).argtypes is not None, "capi.load() gives %s no prototype" % n
    for n, count in ARGS.items():  # the prototype has as many parameters as the header's declaration
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % n, header).group(1)
        assert len(decl.split(",")) == count == len(getattr(L, n).argtypes), (n, decl)
        assert getattr(L, n).restype is None
    assert L.sb_is_initialized() == 0  # loading touched no device


@pytest.mark.parametrize("lib", ["libsparsebench_crs.so", "libsparsebench_scs.so", "libsparsebench_crs_sp.so", "libsparsebench_scs_sp.so"])
def test_dropin_libraries_export_solveCGBatch(lib):
    from sparsebench_amd import hostapi
    hostapi.host()
    hostapi.host("single")
    d = ctypes.CDLL(os.path.join(LIB, lib))
    assert hasattr(d, "solveCGBatch")
    hdr = open(os.path.join(ROOT, "include", "sparsebench", "sparsebench.h")).read()
    assert re.search(r"\bint\s+solveCGBatch\s*\(\s*Comm\s*\*[^)]*Parameter\s*\*[^)]*Matrix\s*\*[^)]*int\s+nrhs\s*\)", hdr)


def test_hostapi_batchcg_refuses_single_precision():
    from sparsebench_amd import hostapi

    class FakeSP:  # never touched: the refusal comes first
        precision = "single"

        def rhs(self):
            raise AssertionError("the library was touched")

    with pytest.raises(ValueError, match="double precision only"):
        hostapi.BatchCG(FakeSP())
    for name in ("solve", "start", "run_iters", "finish", "iterations", "history", "solution", "check_residual",
                 "launches_per_body", "loop_ms", "counters", "free"):
        assert callable(getattr(hostapi.BatchCG, name)), name


def test_driver_help_names_the_option():
    import driver_options as opts
    assert "-n <int>   Number of right-hand sides for -t cg. Default 1." in opts.help_text()
    size = ["-x", "8", "-y", "8", "-z", "8", "-i", "10"]
    for args, nrhs in ((["-t", "cg", "-n", "4"], 4), (["-n", "4"], 4), (["-t", "cg", "-n", "3"], 3), (["-t", "cg"], 1), ([], 1)):
        p = opts.accepted(args + size)  # -n takes an argument and lands in nrhs (a width the layer does not have is its own refusal)
        assert p.type == opts.TYPE["cg"] and p.nrhs == nrhs
    assert opts.accepted(["-t", "cg", "-n", "4"] + size, precision="single").nrhs == 4  # (refused by the solver, not by the options)
    for t in ("spmv", "gmres"):
        opts.refused(["-n", "2", "-t", t] + size, "-n <int> (several right-hand sides) goes with -t cg only\n")
    assert opts.no_device_was_touched()
