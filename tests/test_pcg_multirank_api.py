"""What PCG on several ranks adds to the driver's option check and to the Python interface, without a GPU: which
command lines run under a several-rank launcher and which are refused, with which message; hostapi.PCG's refusal of the one-rank
preconditioners before the library is touched; the help text."""
import ctypes as C
import re

import pytest

import driver_options as opts
from sparsebench_amd import hostapi


def check_ranks(args, size):
    """the command line through sbh_parse_options, then through sbh_check_ranks for `size` ranks: (status, message)"""
    H = opts._lib("double")
    H.sbh_check_ranks.restype = C.c_int
    H.sbh_check_ranks.argtypes = [C.POINTER(opts.Options), C.c_int, C.c_char_p, C.c_size_t]
    words = [b"sparseBench"] + [str(a).encode() for a in args]
    argv = (C.c_char_p * (len(words) + 1))(*words, None)
    param, o, msg = opts.Parameter(), opts.Options(), C.create_string_buffer(4096)
    H.initParameter(C.byref(param))
    assert H.sbh_parse_options(len(words), argv, C.byref(param), C.byref(o), msg, len(msg)) == 0, msg.value
    status = H.sbh_check_ranks(C.byref(o), size, msg, len(msg))
    return status, msg.value.decode()


RUNS = [["-t", "pcg"], ["-t", "pcg", "-p", "jacobi"], ["-t", "pcg", "-p", "poly"], ["-t", "pcg", "-p", "poly", "-d", "5"],
        ["-t", "cg"], ["-t", "spmv"], []]
REFUSED = [(["-t", "pcg", "-p", "sgs"], "SGS: runs on one rank\n"), (["-t", "pcg", "-p", "mg"], "MG: runs on one rank\n"),
           (["-t", "pcg", "-p", "mgfw", "-l", "2"], "MG: runs on one rank\n"), (["-t", "pcg", "-p", "mgpoly"], "MG: runs on one rank\n"),
           (["-t", "pcg", "-p", "mgpoly", "-g"], "MG: runs on one rank\n"), (["-t", "pcg", "-p", "mgpoly", "-a"], "MG: runs on one rank\n"),
           (["-t", "bicgstab"], "BiCGStab: runs on one rank\n"), (["-t", "bicgstab", "-P", "poly"], "BiCGStab: runs on one rank\n"),
           (["-t", "gmres"], "GMRES: runs on one rank\n"), (["-t", "gmres", "-P", "jacobi"], "GMRES: runs on one rank\n")]


@pytest.mark.parametrize("size", [2, 3, 8])
def test_option_check_accepts_jacobi_and_poly_on_several_ranks(size):
    for args in RUNS:
        assert check_ranks(opts.SIZE + args, size) == (0, ""), args
    assert opts.no_device_was_touched()


@pytest.mark.parametrize("args,message", REFUSED)
def test_option_check_refuses_the_one_rank_solvers_on_several_ranks(args, message):
    assert check_ranks(opts.SIZE + args, 2) == (1, message)
    assert check_ranks(opts.SIZE + args, 1) == (0, "")  # one rank: everything the parser accepts runs
    assert opts.no_device_was_touched()


def test_the_parser_itself_is_unchanged_by_the_rank_check():
    """sbh_parse_options knows no rank count: it accepts what it accepted, with the same spec"""
    p = opts.accepted(opts.SIZE + ["-t", "pcg", "-p", "poly", "-d", "5"])
    assert p.type == opts.TYPE["pcg"] and p.spec == (opts.KIND["poly"], 0, 5, opts.COARSE["regenerated"])
    p = opts.accepted(opts.SIZE + ["-t", "pcg", "-p", "sgs"])
    assert p.spec[0] == opts.KIND["sgs"]


def two_rank_problem():
    """a host-only Problem that says it is rank 0 of 2.  (A real one takes two processes and a set-up exchange between them:
    tests/gpu_pcg_multirank_worker.py holds one and checks the same refusal on it; the refusal reads rank and size alone.)"""
    p = hostapi.Problem("generate", 8, 8, 8, fmt="crs", upload=False)
    p.rank, p.size = 0, 2
    return p


@pytest.mark.parametrize("kw", [dict(precond="sgs"), dict(precond="mg", levels=2), dict(precond="mgfw"), dict(precond="mgpoly"),
                                dict(precond="mgpoly", galerkin=True), dict(precond="mgpoly", coarsening="aggregation")])
def test_hostapi_pcg_refuses_the_one_rank_preconditioners_before_the_library(kw):
    p = two_rank_problem()
    with pytest.raises(ValueError, match=r"precond='%s' runs on one rank \(the problem is rank 0 of 2\)" % kw["precond"]):
        hostapi.PCG(p, **kw)
    assert opts.no_device_was_touched()
    p.free()


def test_problem_records_its_rank_and_size():
    p = hostapi.Problem("generate", 8, 8, 8, fmt="crs", upload=False)
    assert (p.rank, p.size) == (0, 1)
    p.free()


def test_help_text_says_what_runs_on_several_ranks():
    help_text = opts.help_text()
    assert re.search(r"Several ranks:.*-t pcg with -p jacobi or -p poly", help_text)
    # the regexes of the existing tests: the help text is still whole
    assert re.search(r"-p <jacobi\|sgs>.*Default jacobi", help_text) and "-C <int>" in help_text
    assert re.search(r"-t <bench type>.*\bbicgstab\b", help_text, re.S) and re.search(r"-t <bench type>.*\bpcg\b", help_text)
    assert re.search(r"-p poly\b", help_text) and re.search(r"-d <int>.*-p poly.*Default 3", help_text)
    assert re.search(r"-P <sgs\|mg\|mgfw\|poly\|mgpoly>.*-t bicgstab", help_text) and re.search(r"-t gmres.*-P jacobi", help_text)
    assert re.search(r"-r <int>   GMRES restart length", help_text)
    assert re.search(r"-a\b.*Smoothed-aggregation coarsening.*-p mgpoly.*any matrix", help_text)
    assert re.search(r"-g\b.*Galerkin coarse operators.*-p mgpoly", help_text)
    assert re.search(r"-p mgpoly\b", help_text) and re.search(r"-p mgpoly.*-l.*-d.*Default 2", help_text, re.S)
