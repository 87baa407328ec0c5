"""What the preconditioner handles of PCG report about themselves, pinned exactly: sb_pcg_precond_bytes
(the byte model every reported GB/s divides), sb_pcg_launches_per_body, the levels and the rows and colours of each, for Jacobi
and SGS over sgs_cases' kernel shapes x formats and for both V-cycles over mg_cases' (plus Sell-4-8).  The values are sums of
integers held in doubles: equality, no tolerance.  tests/golden/precond_bytes.json was recorded from the code as it stood
before the preconditioners' Sell-64 packers and byte formulas were made one (tests/golden/make_golden_precond_bytes.py), so a
change to any term of the model shows here and not only as another GB/s.  Creating the handles is all the test does."""
import json
import os

import pytest

import mg_cases
import pcg_ref
import sgs_cases
from sparsebench_amd import hostapi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "precond_bytes.json")


def matrix_name(matrix):
    return "_".join(os.path.basename(str(v)) for v in matrix)


def cases():
    """[(key, matrix, (fmt, C, sigma), [(precond, levels), ...])]: one Problem each, its handles made on it one after another"""
    out = []
    for matrix in sgs_cases.KERNEL_SHAPES:
        for f in sgs_cases.KERNEL_FORMATS:
            out.append(("%s|%s_%d_%d" % ((matrix_name(matrix),) + f), matrix, f, [("jacobi", None), ("sgs", None)]))
    for matrix, levels in mg_cases.KERNEL_SHAPES:
        for f in mg_cases.KERNEL_FORMATS:
            out.append(("%s|%s_%d_%d" % ((matrix_name(matrix),) + f), matrix, f, [("mg", levels), ("mgfw", levels)]))
    matrix, levels = mg_cases.SELL_4_8_SHAPE
    out.append(("%s|scs_4_8" % matrix_name(matrix), matrix, ("scs", 4, 8), [("mg", levels), ("mgfw", levels)]))
    return out


def record(matrix, fmt, C, sigma, handles, tmp):
    """{precond: what the handle reports} for the handles of one problem"""
    p = hostapi.Problem(*pcg_ref.problem_args(matrix, tmp), fmt=fmt, Cc=C, sigma=sigma)
    out = {}
    for precond, levels in handles:
        s = hostapi.PCG(p, precond=precond, levels=levels)
        L = s.levels()
        out[precond] = dict(precond=s.precond(), bytes=s.precond_bytes(), launches=s.launches_per_body(), levels=L,
                            colours=s.colours(), rows=[s.level_rows(l) for l in range(L)],
                            level_colours=[s.level_colours(l) for l in range(L)])
        s.free()
    p.free()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_the_golden_holds_every_case_and_no_other(golden):
    assert sorted(golden) == sorted(c[0] for c in cases())


@pytest.mark.parametrize("key,matrix,f,handles", cases(), ids=[c[0] for c in cases()])
def test_bytes_launches_and_levels_are_the_recorded_ones(gpu, golden, key, matrix, f, handles, tmp_path):
    got = record(matrix, f[0], f[1], f[2], handles, tmp_path)
    for precond, _ in handles:
        want = golden[key][precond]
        assert got[precond]["bytes"] == float(want["bytes"]) and float(want["bytes"]).is_integer(), (key, precond, got[precond], want)
        assert got[precond] == want, (key, precond)
