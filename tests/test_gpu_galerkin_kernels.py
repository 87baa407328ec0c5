"""sb_matrix_galerkin alone on the GPU == the CPU restatement (tests/galerkin_ref.py, pinned by
tests/test_galerkin_host.py) BIT FOR BIT in row pointers, columns and values, with the counts of sb_csr_stats: stencil grids from
one coarse row ((2, 2, 2)) over a partial wave of rows ((6, 4, 2): 48), exactly two chunks ((8, 4, 4)) and (10, 4, 2) to mg_cases'
(12, 8, 20) and (34, 6, 10), in CRS, Sell-64-1, Sell-64-256 and (8^3) Sell-4-8 with the product identical across the formats; the
scaled 8^3 matrix whose products are not exact; exact cancellation and underflow with their dropped counts; a hand-made P with an
empty row, a stored 0.0, the same column twice in one row and a coarse column no fine row touches; a row of exactly the capacity's
1024 distinct columns, and one more refused in a child process.  The launches are one workgroup per output row, neither capped nor
grid-strided: there is no second trip to reach."""
import os
import subprocess
import sys

import numpy as np
import pytest

import galerkin_ref as gr
import mg_cases
from conftest import load_json
from sparsebench_amd import hostapi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRIDS = [(2, 2, 2), (6, 4, 2), (8, 4, 4), (10, 4, 2), (12, 8, 20), (34, 6, 10)]
assert {("dims",) + g for g in GRIDS[-2:]} <= {m for m, _ in mg_cases.KERNEL_SHAPES}


def check_stats(st, dropped, maxima, what):
    assert st["dropped"] == dropped and (st["max_row_t"], st["max_row_ac"]) == tuple(maxima), (what, st, dropped, maxima)
    assert st["stage1_ms"] > 0.0 and st["stage2_ms"] > 0.0 and st["t_entries"] >= st["max_row_t"], (what, st)


@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(str(v) for v in d))
def test_stencil_product_equals_the_restatement_in_every_format(gpu, dims):
    P = hostapi.mg_trilinear(*dims)
    nc = dims[0] * dims[1] * dims[2] // 8
    want, dropped, maxima = gr.product(gr.stencil(dims), P, nc)
    assert dropped == 0 and len(want[0]) == nc + 1
    for fmt, C, sigma in mg_cases.KERNEL_FORMATS:
        p = hostapi.Problem("generate", *dims, fmt=fmt, Cc=C, sigma=sigma)
        got, st = hostapi.galerkin_product(p, P)
        gr.same_csr(got, want, (dims, fmt, C, sigma))
        check_stats(st, dropped, maxima, (dims, fmt, C, sigma))
        p.free()


def test_sell_4_8_and_the_golden(gpu):
    P = hostapi.mg_trilinear(8, 8, 8)
    want = gr.product(gr.stencil((8, 8, 8)), P, 64)[0]
    assert gr.digest(want) == {k: load_json("galerkin_hist.json")["products"]["hpcg8_L3"][0][k] for k in ("nnz", "sha256")}
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=4, sigma=8)
    assert not np.array_equal(p.array("oldToNewPerm"), np.arange(512))  # a real permutation
    gr.same_csr(hostapi.galerkin_product(p, P)[0], want, "Sell-4-8")
    p.free()


@pytest.mark.parametrize("fmt,C,sigma", mg_cases.KERNEL_FORMATS + [("scs", 4, 8)])
def test_inexact_products_equal_the_restatement(gpu, fmt, C, sigma):
    A, P = gr.scaled_hpcg8(), hostapi.mg_trilinear(8, 8, 8)
    want, dropped, maxima = gr.product(A, P, 64)
    assert gr.digest(want) == {k: load_json("galerkin_hist.json")["products"]["scaled8"][0][k] for k in ("nnz", "sha256")}
    p = hostapi.Problem.from_csr(*A, fmt=fmt, Cc=C, sigma=sigma)
    got, st = hostapi.galerkin_product(p, P)
    gr.same_csr(got, want, ("scaled 8^3", fmt, C, sigma))
    check_stats(st, dropped, maxima, ("scaled 8^3", fmt))
    p.free()


@pytest.mark.parametrize("case", ["cancelling", "underflowing"])
@pytest.mark.parametrize("fmt,sigma", [("crs", 1), ("scs", 256)])
def test_cancellation_and_underflow_are_dropped_and_counted(gpu, case, fmt, sigma):
    A, P, nc = getattr(gr, case)()
    want, dropped, maxima = gr.product(A, P, nc)
    assert dropped >= 1 and len(want[1]) >= 1
    p = hostapi.Problem.from_csr(*A, fmt=fmt, Cc=64, sigma=sigma)
    got, st = hostapi.galerkin_product(p, P)
    gr.same_csr(got, want, (case, fmt))
    check_stats(st, dropped, maxima, (case, fmt))
    p.free()


def hand_made_p():
    """10 x 5 on the (10, 1, 1)-like chain below: row 3 empty, a stored 0.0 in row 4, column 1 twice in row 5 (and column 2 twice
    in row 6, once with 0.0), coarse column 4 touched by no fine row"""
    rows = [[(0, 1.0)], [(0, 0.5), (1, 0.5)], [(1, 1.0)], [], [(1, 0.0), (2, 0.75)], [(1, 0.25), (2, 0.5), (1, 0.125)],
            [(2, 0.0), (3, 1.0), (2, 0.3)], [(3, 0.7), (2, 0.1)], [(3, 1.0)], [(3, 0.5), (0, -0.5)]]
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    col = np.array([c for r in rows for c, _ in r], dtype=np.uint32)
    val = np.array([w for r in rows for _, w in r], dtype=np.float64)
    return ptr, col, val


@pytest.mark.parametrize("fmt,C,sigma", mg_cases.KERNEL_FORMATS + [("scs", 4, 8)])
def test_a_hand_made_p_with_an_empty_row_a_zero_a_repeated_column_and_an_untouched_coarse_column(gpu, fmt, C, sigma):
    n = 10
    ent = [(i, j, (3.0 + 0.1 * i if i == j else -1.0 / (1 + i + j))) for i in range(n) for j in range(n) if abs(i - j) <= 2 - (i % 2)]
    ent[7] = (ent[7][0], ent[7][1], 0.0)  # an explicit zero of A
    ptr = np.zeros(n + 1, dtype=np.uint64)
    for i, _, _ in ent:
        ptr[i + 1] += 1
    A = (np.cumsum(ptr).astype(np.uint64), np.array([j for _, j, _ in ent], dtype=np.uint32), np.array([v for _, _, v in ent]))
    P = hand_made_p()
    want, dropped, maxima = gr.product(A, P, 5)
    assert want[0][5] == want[0][4] and want[0][4] > want[0][3]  # the untouched coarse column: an empty last row
    assert not np.any(want[1] == 4)
    p = hostapi.Problem.from_csr(*A, fmt=fmt, Cc=C, sigma=sigma)
    got, st = hostapi.galerkin_product(p, P, n_coarse=5)
    gr.same_csr(got, want, ("hand made", fmt, C, sigma))
    check_stats(st, dropped, maxima, ("hand made", fmt))
    p.free()


def wide_p(ncols):
    """2 x (ncols + 1): row 0 has `ncols` distinct columns in a scrambled order, row 1 the last one"""
    order = (np.arange(ncols, dtype=np.uint64) * 389) % ncols  # 389 is prime to 1024 and to 1025
    assert len(set(order.tolist())) == ncols
    ptr = np.array([0, ncols, ncols + 1], dtype=np.uint64)
    col = np.concatenate([order, [ncols]]).astype(np.uint32)
    val = np.concatenate([1.0 + np.arange(ncols) / 1024.0, [2.0]])
    return ptr, col, val


def identity2():
    return np.array([0, 1, 2], dtype=np.uint64), np.array([0, 1], dtype=np.uint32), np.array([1.0, 1.0])


def test_a_row_of_exactly_the_capacity_passes(gpu):
    A, P = identity2(), wide_p(1024)
    want, dropped, maxima = gr.product(A, P, 1025)
    assert maxima == (1024, 1024) and dropped == 0
    p = hostapi.Problem.from_csr(*A, fmt="crs")
    got, st = hostapi.galerkin_product(p, P)
    gr.same_csr(got, want, "capacity")
    check_stats(st, dropped, maxima, "capacity")
    p.free()


CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
from sparsebench_amd import capi, hostapi
import numpy as np
import test_gpu_galerkin_kernels as t
what = sys.argv[1]
capi.init(0)
if what == "capacity":
    p = hostapi.Problem.from_csr(*t.identity2(), fmt="crs")
    hostapi.galerkin_product(p, t.wide_p(1025))
print("NOT REFUSED")
"""


def test_one_column_above_the_capacity_is_refused_not_truncated(gpu):
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), "capacity"], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    err = out.stderr.decode()
    assert out.returncode == 1, (out.returncode, err[-1000:])
    assert "sb_matrix_galerkin: stage 1 (A P): row 0 has at least 1025 distinct columns, the capacity of a row is 1024" in err, err[-1000:]
    assert "sbhip:" in err and "NOT REFUSED" not in out.stdout.decode()
    assert "illegal memory access" not in err and "HIP error" not in err
