"""The single-precision CG loop on the MI355X at row counts off the 4 / 64 / 256 grids (tests/sp_odd_cases.py): k, the r.r and
p.Ap histories and x bit for bit against sp_ref.cg over sp_ref.spmv_crs, in the tree order (fused and unfused; for sigma = 256
restated in the device's permuted row order) and in the seq order (at (33, 7, 5) and (19, 21, 23) also against the reference's
own SP history, tests/golden/cg_hist_sp_ref_odd.json), a solve in pieces, and the same through the opt-in mirror.  No tolerance
anywhere; NaN compares as NaN."""
import json
import os

import numpy as np
import pytest

import sp_odd_cases as oc
from sp_odd_cases import bits, equal_runs
from sparsebench_amd import capi, hostapi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_ODD = os.path.join(ROOT, "tests", "golden", "cg_hist_sp_ref_odd.json")
FORMATS = [("crs", 1), ("scs", 1), ("scs", 256)]
CASES = [(s, f, g) for s in oc.SHAPES for (f, g) in FORMATS if s != oc.BIG or (f, g) != ("scs", 1)]
name_of = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # test ids: 33x7x5-scs-256


@pytest.fixture(scope="module", autouse=True)
def gpu():
    capi.init(0)


@pytest.fixture(scope="module")
def restated():
    """shape -> its Restatement: every sp_ref history is computed once per shape (and row order), not once per format"""
    kept = {}

    def get(shape):
        if shape not in kept:
            itermax = oc.SHAPES[shape][0] if shape in oc.SHAPES else oc.MIRROR_SHAPES[shape]
            kept[shape] = oc.Restatement(shape, itermax)
        return kept[shape]

    return get


def problem(shape, fmt, sigma, precision="single", mirror=None):
    return hostapi.Problem("generate", shape[0], shape[1], shape[2], fmt=fmt, Cc=64, sigma=sigma, precision=precision, mirror=mirror)


def solve(p, itermax, order, **kw):
    cg = hostapi.CG(p, dot_order=order, **kw)
    k = cg.solve(itermax)
    rr, pap = cg.history()
    x = cg.solution()
    cg.free()
    return k, rr, pap, x


def device_order(p, fmt, sigma):
    """oldToNewPerm where the device's row order is not the caller's"""
    return p.array("oldToNewPerm").copy() if fmt == "scs" and sigma > 1 else None


def check_against(got, ref, what):
    """k, both histories and x; and the exact r.r = 0 exit (`normr > eps` fails on the device) wherever sp_ref takes it"""
    assert got[0] == ref[0], (what, got[0], ref[0])
    assert np.array_equal(bits(got[1]), bits(ref[1])), (what, "r.r")
    assert np.array_equal(bits(got[2]), bits(ref[2])), (what, "p.Ap")
    assert got[3].dtype == np.float32 and np.array_equal(bits(got[3]), bits(ref[3])), (what, "x")
    if ref[1][-1] == 0.0:
        assert got[1][-1] == 0.0 and got[0] == len(got[1]) + 1, what


def test_the_shapes_are_what_the_table_says(restated):
    for shape, (itermax, rows, l1) in oc.SHAPES.items():
        assert shape[0] * shape[1] * shape[2] == rows and (rows + 255) // 256 == l1 and rows % 4 != 0
    r = restated((33, 7, 5))
    assert r.nr == 1155
    # the two orders cannot be confused, and the small shapes leave through an exact r.r = 0
    assert not equal_runs(r.tree(), r.seq())
    assert restated((5, 5, 5)).tree()[0] == 27 and restated((5, 5, 5)).seq()[0] == 28
    assert restated((5, 5, 5)).tree()[1][-1] == 0.0 and restated((7, 7, 6)).seq()[1][-1] == 0.0


@pytest.mark.parametrize("shape,fmt,sigma", CASES, ids=name_of)
def test_tree_history_and_x_are_sp_refs_fused_and_unfused(restated, shape, fmt, sigma):
    itermax = oc.SHAPES[shape][0]
    p = problem(shape, fmt, sigma)
    assert p.nr == oc.SHAPES[shape][1]
    fused = solve(p, itermax, "tree")
    unfused = solve(p, itermax, "tree", fused=False)
    ref = restated(shape).tree(device_order(p, fmt, sigma))
    p.free()
    check_against(fused, ref, (shape, fmt, sigma, "fused"))
    check_against(unfused, ref, (shape, fmt, sigma, "unfused"))
    assert equal_runs(fused, unfused)
    assert not np.isnan(ref[1]).any() and not np.isnan(ref[2]).any()


@pytest.mark.parametrize("shape,fmt,sigma", [c for c in CASES if c[0] != oc.BIG], ids=name_of)
def test_seq_history_and_x_are_sp_refs_and_the_references(restated, shape, fmt, sigma):
    itermax = oc.SHAPES[shape][0]
    p = problem(shape, fmt, sigma)
    got = solve(p, itermax, "seq")
    p.free()
    ref = restated(shape).seq()
    check_against(got, ref, (shape, fmt, sigma, "seq"))
    assert not equal_runs(ref, restated(shape).tree())
    if shape in ((33, 7, 5), (19, 21, 23)):  # the reference's own SP solveCG at this shape
        name = "hpcg%dx%dx%d" % shape
        g = json.load(open(GOLDEN_ODD))[name]
        assert g["itermax"] == itermax and got[0] == g["k"]
        assert np.array_equal(bits(got[1]), bits([float(v) for v in g["rr"]])), name
        assert np.array_equal(bits(got[2]), bits([float(v) for v in g["pAp"]])), name


@pytest.mark.parametrize("fmt,sigma", FORMATS)
@pytest.mark.parametrize("pieces", [(7, 53), (1, 58, 1)], ids=name_of)
def test_a_solve_in_pieces_is_one_solve(restated, fmt, sigma, pieces):
    """(33, 7, 5) as 7 + 53 iterations: every piece ends with its beta step flushed, the next p update pays the owed x += alpha p
    (x_pending) over a partial float4, and finish pays the last one (cg_x_finalize_f32)"""
    shape, itermax = (33, 7, 5), 60
    p = problem(shape, fmt, sigma)
    whole = solve(p, itermax, "tree")
    cg = hostapi.CG(p, dot_order="tree")
    cg.start(itermax, 0.0)
    for n in pieces:
        cg.run_iters(n)
    k = cg.finish()
    rr, pap = cg.history()
    got = (k, rr, pap, cg.solution())
    cg.free()
    ref = restated(shape).tree(device_order(p, fmt, sigma))
    p.free()
    assert equal_runs(got, whole), pieces
    check_against(got, ref, (shape, fmt, sigma, pieces))


@pytest.mark.parametrize("shape", sorted(oc.MIRROR_SHAPES), ids=name_of)
@pytest.mark.parametrize("fmt,sigma", FORMATS)
def test_the_loop_through_the_mirror_where_it_is_built(restated, monkeypatch, shape, fmt, sigma):
    """with the switch on the matrix has all row programs exactly where its fp64 twin has; built (the 3-launch loop over
    spmv_prog_fusep_f32, fuse_p off, the seq order's spmv_prog_f32) or not (the streaming kernels), the loop gives sp_ref's
    k, histories and x.  The run prints which it was"""
    monkeypatch.setenv("SB_PLACE", "0")  # the fp64 twin is uploaded for its structure only
    itermax = oc.MIRROR_SHAPES[shape]
    q = problem(shape, fmt, sigma, precision="double")
    want = q.all_row_programs()
    q.free()
    p = problem(shape, fmt, sigma, mirror=True)
    built = p.all_row_programs()
    print("SP mirror at %s %s sigma %d: all_row_programs = %d (fp64: %d), mode %d" % (shape, fmt, sigma, built, want, p.pack_info()["mode"]))
    assert built == want
    assert p.pack_info()["mode"] == (5 if built else 0)
    cg = hostapi.CG(p, dot_order="tree")
    assert cg.fuse_p() == built and cg.launches_per_body() == (3 if built or fmt == "scs" else 4)
    cg.free()
    r = restated(shape)
    tree = r.tree(device_order(p, fmt, sigma))
    check_against(solve(p, itermax, "tree"), tree, (shape, fmt, sigma, "tree"))
    check_against(solve(p, itermax, "tree", fuse_p=0), tree, (shape, fmt, sigma, "tree, fuse_p off"))
    check_against(solve(p, itermax, "tree", fused=False), tree, (shape, fmt, sigma, "tree, unfused"))
    check_against(solve(p, itermax, "seq"), r.seq(), (shape, fmt, sigma, "seq"))
    p.free()
