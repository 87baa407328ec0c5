"""Pins tests/cg_kernels_ref.py -- the CG loop's kernels restated launch by launch, the yardstick of
tests/test_gpu_cg_kernels.py -- on the CPU: the restated launches chained in the order sb_cg_start / loop_body / sb_cg_finish
enqueue them reproduce k, both histories and x of solveCG's restatement (tests/cg_batch_ref.py, itself pinned to the oracle's CG)
bit for bit.  Three op lists: the default one on one rank (alpha folded into the r update, beta into the next p update), the
separate scalar launches, and the reference-shaped list (dot_spans / waxpby_sdev)."""
import numpy as np
import pytest

from oracle import pyoracle as po

import cg_batch_ref
import cg_kernels_ref as ck

SHAPES = [(16, 12, 10), (33, 7, 5)]


def chain(op, b, itermax, eps, how):
    """the launches of one sb_cg_solve; every body is enqueued whether or not the loop has exited, as on the device"""
    n = len(b)
    m = ck.groups(n)
    cap = itermax + 2
    S = ck.Block(itermax=itermax, eps=eps, hist_cap=cap)
    rr_hist, pAp_hist = np.full(cap, -1.0), np.full(cap, -1.0)
    x = np.zeros(n)
    p = po.waxpby(1.0, x, 0.0, x)
    Ap = op.spmv(p)
    r = np.zeros(n)
    if how == "oplist":
        r = po.waxpby(1.0, b, -1.0, Ap)
        q = ck.level0(r, r)
    else:
        _, r, q = ck.dot_spans(2, S, b, Ap, None, r, stop=False)
    S, rr_hist, pAp_hist = ck.scalar(0, True, S, q, m, 0, 0, 0, rr_hist, pAp_hist)
    l1rr, l1pAp, owing = None, None, False
    for k in range(1, itermax):
        if k == 1:
            S, p, _, _ = ck.update_p(0, S, r, p, None, 1)
        elif how == "oplist":
            if not S.stop:
                q = ck.level0(r, r)
            S, rr_hist, pAp_hist = ck.scalar(1, True, S, q, m, 0, 0, 0, rr_hist, pAp_hist)
            S, p, _, _ = ck.update_p(0, S, r, p, None, 0)
        elif owing:
            S, p, x, rr_hist = ck.update_p(1, S, r, p, x, 0, m, l1rr, rr_hist)
            owing = False
        else:
            S, p, x, _ = ck.update_p(0, S, r, p, x, 0)
        if not S.stop:  # (the SpMV and its dot return at once on a set flag)
            Ap = op.spmv(p)
            l1pAp = ck.level0(p, Ap) if how == "oplist" else po.ddot_partials(p, Ap)
        if how == "oplist":
            S, rr_hist, pAp_hist = ck.scalar(2, True, S, l1pAp, m, 0, 0, 0, rr_hist, pAp_hist)
            w = ck.waxpby_sdev(S, x, p, 0)
            x = x if w is None else w
            w = ck.waxpby_sdev(S, r, Ap, 1)
            r = r if w is None else w
            continue
        if how == "folded":
            S, r, l1, rr_hist, pAp_hist = ck.update_r(1, S, Ap, r, m, l1pAp, rr_hist, pAp_hist)
        else:
            S, rr_hist, pAp_hist = ck.scalar(2, True, S, l1pAp, m, 0, 0, 1, rr_hist, pAp_hist)
            S, r, l1, _, _ = ck.update_r(0, S, Ap, r)
        l1rr = l1rr if l1 is None else l1
        assert l1 is None or len(l1) == m
        if how == "folded":
            owing = True  # the beta step rides at the head of the next p update
        else:
            S, rr_hist, pAp_hist = ck.scalar(1, True, S, l1rr, m, 0, 1, 1, rr_hist, pAp_hist)
    if owing:  # flush_beta_fold: nobody comes after the last body
        S, rr_hist, pAp_hist = ck.scalar(1, True, S, l1rr, m, 0, 1, 1, rr_hist, pAp_hist)
    x = ck.x_finalize(S, x, p, p)
    return dict(k=S.iters + 1, rr=rr_hist[:S.n_rr], pAp=pAp_hist[:S.n_pAp], x=x, S=S, tails=(rr_hist[S.n_rr:], pAp_hist[S.n_pAp:]))


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def problem(request):
    g = po.GMatrix.generate(*request.param)
    op = cg_batch_ref.operator(g)
    b = op.to_dev(g.rhs())
    want = {(itermax, eps): cg_batch_ref.solve(op, g.rhs(), itermax, eps) for itermax, eps in ((40, 0.0), (150, 1e-6), (1, 0.0), (2, 0.0))}
    yield op, b, want
    g.free()


@pytest.mark.parametrize("how", ["folded", "separate", "oplist"])
@pytest.mark.parametrize("itermax,eps", [(40, 0.0), (150, 1e-6), (1, 0.0), (2, 0.0)])
def test_chained_launches_equal_the_restatement_of_solveCG(problem, how, itermax, eps):
    op, b, want = problem
    want = want[(itermax, eps)]
    got = chain(op, b, itermax, eps, how)
    assert got["k"] == want["k"], (got["k"], want["k"])
    if eps > 0.0:
        assert 1 < want["k"] < itermax and got["S"].stop == 1  # the loop test on the norm is what ended it
    assert cg_batch_ref.same_bits(got["rr"], want["rr"]), "rr history"
    assert cg_batch_ref.same_bits(got["pAp"], want["pAp"]), "pAp history"
    assert cg_batch_ref.same_bits(got["x"], op.to_dev(want["x"])), "x"
    assert all(np.all(t == -1.0) for t in got["tails"]), "a history entry behind its counter was written"


def test_level0_and_level1_are_the_oracles_partials():
    rng = np.random.default_rng(5)
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1000):
        x, y = rng.standard_normal(n), rng.standard_normal(n)
        q = ck.level0(x, y)
        assert len(q) == 4 * ck.groups(n)
        assert cg_batch_ref.same_bits(ck.level1(q), po.ddot_partials(x, y))
        assert ck.total_of(q, ck.groups(n), 0) == po.ddot_tree(x, y) == ck.total_of(ck.level1(q), ck.groups(n), 1)


def test_hist_cap_guard_and_snapshots():
    """cg_apply: no history store at n_rr == hist_cap / n_pAp == hist_cap while the counters advance; the alpha step copies
    rr / iters / stop_next into snap_*; a stopped or failed step leaves what it must"""
    S = ck.Block(rr=4.0, iters=3, itermax=10, eps=1e-3, n_rr=2, n_pAp=2, hist_cap=2, stop_next=0)
    h = np.array([7.0, 8.0])
    o, rh, ph = ck.cg_apply(1, S, 1.0, h, h, 1)
    assert rh is h and o.n_rr == 3 and o.iters == 4 and o.beta == 0.25 and o.rr_old == 4.0 and o.x_pending == 1 and o.stop == 0
    o, rh, ph = ck.cg_apply(2, S, 8.0, h, h, 0)
    assert ph is h and o.n_pAp == 3 and o.alpha == 0.5 and o.neg_alpha == -0.5 and (o.snap_rr, o.snap_iters, o.snap_stop_next) == (4.0, 3, 0)
    o, rh, ph = ck.cg_apply(1, S.copy(iters=8), 1.0, h, h, 0)
    assert o.iters == 9 and o.stop == 0
    o, rh, ph = ck.cg_apply(1, S.copy(iters=9), 1.0, h, h, 0)
    assert o.stop == 1 and o.iters == 9 and o.n_rr == 2 and o.rr == 4.0 and o.x_pending == 0
    o, rh, ph = ck.cg_apply(0, ck.Block(itermax=1, eps=0.0, hist_cap=4), 9.0, np.zeros(4), None, 0)
    assert o.stop == 1 and o.iters == 0 and o.rr == 9.0 and rh[0] == 9.0 and o.n_rr == 1
    # the fold kernels: vectors from the snapshot, the recorded step from the live fields
    r, p, x = np.array([1.0, 2.0]), np.array([3.0, 5.0]), np.array([0.5, 0.25])
    S = ck.Block(rr=4.0, snap_rr=2.0, iters=3, snap_iters=3, itermax=10, local=1.0, alpha=2.0, hist_cap=0)
    o, pn, xn, _ = ck.update_p(2, S, r, p, x, 0)
    assert o.beta == 0.25 and np.array_equal(pn, r + 0.5 * p) and np.array_equal(xn, x + 2.0 * p)
    o, pn, xn, _ = ck.update_p(2, S.copy(snap_stop_next=1), r, p, x, 0)
    assert pn is p and xn is x and o.iters == 4 and o.stop == 0  # (the live test passed, the snapshot's failed)
    o, pn, xn, _ = ck.update_p(2, S.copy(stop=1), r, p, x, 0)
    assert pn is p and xn is x and o.d().tobytes() == S.copy(stop=1).d().tobytes() and np.array_equal(o.i(), S.copy(stop=1).i())


ENTRIES = {"sb_cg_update_p_native": 11, "sb_cg_update_r_native": 11, "sb_cg_scalar_native": 11, "sb_cg_x_finalize_native": 6,
           "sb_cg_dot_spans_native": 9, "sb_waxpby_sdev_native": 7, "sb_cg_update_p_launch": 2, "sb_cg_update_r_launch": 3}


def test_entries_declared_exported_and_listed():
    """the blocking entries and launch queries: in include/sbhip.h, exported by the library, listed in capi with a prototype of
    as many parameters as the declaration; the control block is 9 doubles and 11 ints as the header says"""
    import ctypes
    import os
    import re
    from sparsebench_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sbhip.h")).read()
    L = capi.load()
    for name, count in ENTRIES.items():
        decl = re.search(r"\b(int|void) %s\s*\(([^)]*)\)" % name, header)
        assert decl, name
        assert name in capi.SYMBOLS and hasattr(L, name)
        fn = getattr(L, name)
        assert len(decl.group(2).split(",")) == count == len(fn.argtypes), (name, decl.group(2))
        assert fn.restype is (ctypes.c_int if decl.group(1) == "int" else None)
    assert len(ck.FIELDS_D) == 9 and len(ck.FIELDS_I) == 11
    assert "blk_d[9] = {%s}" % ", ".join(ck.FIELDS_D) in " ".join(header.replace(" *", " ").split())
    assert "blk_i[11] = {%s}" % ", ".join(ck.FIELDS_I) in " ".join(header.replace(" * ", " ").split())
    assert L.sb_is_initialized() == 0  # loading touched no device
