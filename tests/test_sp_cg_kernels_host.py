"""Pins tests/sp_cg_kernels_ref.py -- the single-precision CG loop's kernels restated launch by launch, the yardstick of
tests/test_gpu_sp_cg_kernels.py -- on the CPU: the restated launches chained in the orders sp_cg_start / sp_loop_body /
sp_cg_finish enqueue them reproduce k, both histories and x of sp_ref.cg (the SP build's solveCG, tied to the reference's recorded
histories by the whole-solve tests) bit for bit.  Four orders: the reference-shaped op list, the fused loop on one rank (beta step
at the head of the next p update, alpha step in the r update), the fused loop with the p update inside the SpMV (double-buffered
p, the beta step a launch of its own) and the split order of the communicator's plane (local reduce | apply)."""
import numpy as np
import pytest

from oracle import pyoracle as po

import sp_cg_kernels_ref as ck
import sp_ref

F = np.float32
SHAPES = [(16, 12, 10), (33, 7, 5)]
CASES = [(40, 0.0), (41, 0.0), (150, 1e-3), (1, 0.0), (2, 0.0), (3, 0.0)]
SENTINEL = F(-7.5)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def split_scalar(mode, S, q, m, defer_x, rr_hist, pAp_hist, carried):
    """the step as local reduce | (all-reduce of one rank: the value itself) | apply"""
    loc = ck.local(S, q, m, 1, carried)
    S, rr_hist, pAp_hist = ck.apply_local(mode, S, loc, defer_x, rr_hist, pAp_hist)
    return S, rr_hist, pAp_hist, loc


def chain(spmv, b, itermax, eps, how):
    """the launches of one solve; every body is enqueued whether or not the loop has exited, as on the device"""
    b = np.ascontiguousarray(b, dtype=F)
    n = len(b)
    m = ck.groups(n)
    cap = itermax + 2
    S = ck.Block(itermax=itermax, eps=eps, hist_cap=cap)
    rr_hist, pAp_hist = np.full(cap, SENTINEL), np.full(cap, SENTINEL)
    x = np.zeros(n, F)
    p = sp_ref.waxpby(1.0, x, 0.0, x)
    Ap = spmv(p)
    r = sp_ref.waxpby(1.0, b, -1.0, Ap)
    S, rr_hist, pAp_hist = ck.scalar(0, S, sp_ref.level0(r, r), m, 0, 0, rr_hist, pAp_hist)
    pb = [p, np.zeros(n, F)]  # (fusep: body k leaves p_k in buffer k & 1)
    l1rr, l1pAp, q, owing, loc = None, None, None, False, SENTINEL
    for k in range(1, itermax):
        if how == "oplist":
            if k == 1:
                S, p, _, _ = ck.update_p(0, S, r, p, None, 1)
            else:
                if not S.stop:
                    q = sp_ref.level0(r, r)
                S, rr_hist, pAp_hist = ck.scalar(1, S, q, m, 0, 0, rr_hist, pAp_hist)
                S, p, _, _ = ck.update_p(0, S, r, p, None, 0)
            if not S.stop:  # (the SpMV and the dot return at once on a set flag)
                Ap = spmv(p)
                q = sp_ref.level0(p, Ap)
            S, rr_hist, pAp_hist = ck.scalar(2, S, q, m, 0, 0, rr_hist, pAp_hist)
            w = ck.axpy_sdev(S, x, p, 0)
            x = x if w is None else w
            w = ck.axpy_sdev(S, r, Ap, 1)
            r = r if w is None else w
            continue
        if how == "fusep":  # the p update inside the SpMV: cg_update_p_f32<0>'s arithmetic from buffer (k - 1) & 1 into k & 1
            S, pn, x, _ = ck.update_p(0, S, r, pb[(k - 1) & 1], x, int(k == 1))
            if not S.stop:
                pb[k & 1] = p = pn
        elif k == 1:
            S, p, _, _ = ck.update_p(0, S, r, p, None, 1)
        elif owing:
            S, p, x, rr_hist = ck.update_p(1, S, r, p, x, 0, m, l1rr, rr_hist)
            owing = False
        else:
            S, p, x, _ = ck.update_p(0, S, r, p, x, 0)
        if not S.stop:
            Ap = spmv(p)
            l1pAp = ck.dot_l1(p, Ap, 0)
        if how == "split":
            S, rr_hist, pAp_hist, loc = split_scalar(2, S, l1pAp, m, 0, rr_hist, pAp_hist, loc)
            S, r, l1, _, _ = ck.update_r(0, S, Ap, r)
        else:
            S, r, l1, rr_hist, pAp_hist = ck.update_r(1, S, Ap, r, m, l1pAp, rr_hist, pAp_hist)
        l1rr = l1rr if l1 is None else l1
        assert l1 is None or len(l1) == m
        if how == "fused":
            owing = True  # the beta step rides at the head of the next p update
        elif how == "fusep":
            S, rr_hist, pAp_hist = ck.scalar(1, S, l1rr, m, 1, 1, rr_hist, pAp_hist)
        else:
            S, rr_hist, pAp_hist, loc = split_scalar(1, S, l1rr, m, 1, rr_hist, pAp_hist, loc)
    if owing:  # sp_flush_beta: nobody comes after the last body
        S, rr_hist, pAp_hist = ck.scalar(1, S, l1rr, m, 1, 1, rr_hist, pAp_hist)
    x = ck.x_finalize(S, x, pb[0], pb[1]) if how == "fusep" else ck.x_finalize(S, x, p)
    return dict(k=S.iters + 1, rr=rr_hist[:S.n_rr], pAp=pAp_hist[:S.n_pAp], x=x, S=S, tails=(rr_hist[S.n_rr:], pAp_hist[S.n_pAp:]))


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def problem(request):
    g = po.GMatrix.generate(*request.param)
    rp, col, val = g.rowPtr.copy(), g.col.copy(), g.val.astype(F)
    b = g.rhs().astype(F)
    g.free()

    def spmv(v):
        return sp_ref.spmv_crs(rp, col, val, v)

    want = {c: sp_ref.cg(spmv, b, *c) for c in CASES}
    return spmv, b, want


@pytest.mark.parametrize("how", ["fused", "fusep", "split", "oplist"])
@pytest.mark.parametrize("itermax,eps", CASES)
def test_chained_launches_equal_sp_ref_cg(problem, how, itermax, eps):
    spmv, b, want = problem
    k, rr, pAp, x = want[(itermax, eps)]
    got = chain(spmv, b, itermax, eps, how)
    assert got["k"] == k, (got["k"], k)
    S = got["S"]
    if eps > 0.0:  # the loop test on the norm is what ended it
        assert 1 < k < itermax and S.stop == 1 and S.stop_next == 1
    elif itermax > 1:  # ... and here itermax
        assert k == itermax and S.stop_next == 0
    assert same_bits(got["rr"], rr), "rr history"
    assert same_bits(got["pAp"], pAp), "pAp history"
    assert same_bits(got["x"], x), "x"
    assert S.n_pAp == k - 1 and len(rr) == max(k - 1, 1)
    assert all(np.all(bits(t) == bits(SENTINEL)) for t in got["tails"]), "a history entry behind its counter was written"


def test_double_buffered_finalize_takes_the_last_bodys_buffer(problem):
    """itermax 40 and 41 end on an odd and an even n_pAp: cg_x_finalize2_f32 reads p1 / p0, which differ"""
    spmv, b, _ = problem
    for itermax, odd in ((40, 1), (41, 0)):
        S = chain(spmv, b, itermax, 0.0, "fusep")["S"]
        assert S.n_pAp & 1 == odd and S.x_pending == 1
    x, p0, p1 = np.arange(3, dtype=F), np.full(3, 2.0, F), np.full(3, 4.0, F)
    S = ck.Block(alpha=0.5, x_pending=1, n_pAp=3)
    assert same_bits(ck.x_finalize(S, x, p0, p1), x + F(2.0)) and same_bits(ck.x_finalize(S.copy(n_pAp=4), x, p0, p1), x + F(1.0))
    assert same_bits(ck.x_finalize(S, x, p0), x + F(1.0)) and ck.x_finalize(S.copy(x_pending=0), x, p0, p1) is x


def test_totals_are_sp_refs_tree():
    rng = np.random.default_rng(5)
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1000, 300000):
        x, y = rng.standard_normal(n).astype(F), rng.standard_normal(n).astype(F)
        q = sp_ref.level0(x, y)
        m = ck.groups(n)
        assert len(q) == 4 * m and len(ck.level1_of(x, y)) == m
        assert bits(ck.total_of(q, m, 0)) == bits(sp_ref.dot_tree(x, y)) == bits(ck.total_of(ck.level1_of(x, y), m, 1))
    assert bits(ck.total_of(None, 0, 1)) == 0  # no values: +0.0


def test_the_float_steps_as_the_kernels_take_them():
    """cg_apply_f32 and the fold kernels' own reads: the quotient rounded to float before the double carries it, -(rr / total)
    against neg_alpha, the snapshot against the live fields, the hist_cap guard, defer_x, normr_fails"""
    h = np.array([7.0, 8.0], F)
    S = ck.Block(rr=3.0, iters=3, itermax=10, eps=1e-3, n_rr=2, n_pAp=2, hist_cap=2)
    o, rh, ph = ck.cg_apply(1, S, 1.0, h, h, 1)
    assert o.beta == np.float64(F(1.0) / F(3.0)) != 1.0 / 3.0 and rh is h and o.n_rr == 3 and o.iters == 4 and o.x_pending == 1
    assert o.rr_old == F(3.0) and o.rr == F(1.0) and o.stop == 0 and o.stop_next == 0
    o, rh, ph = ck.cg_apply(2, S, 7.0, h, h, 0)
    assert ph is h and o.n_pAp == 3 and o.alpha == F(3.0) / F(7.0) and o.neg_alpha == -o.alpha and o.pAp == F(7.0)
    assert (o.snap_rr, o.snap_iters, o.snap_stop_next) == (F(3.0), 3, 0)
    o, rh, ph = ck.cg_apply(1, S.copy(iters=9), 1.0, h, h, 0)
    assert o.stop == 1 and o.iters == 9 and o.n_rr == 2 and o.rr == F(3.0) and o.x_pending == 0
    o, rh, ph = ck.cg_apply(1, S.copy(stop_next=1, hist_cap=4), 1.0, h, h, 1)
    assert o.stop == 1 and o.x_pending == 1 and rh is h
    o, rh, ph = ck.cg_apply(0, ck.Block(itermax=1, eps=0.0, hist_cap=4), 9.0, np.zeros(4, F), None, 0)
    assert o.stop == 1 and o.iters == 0 and o.rr == F(9.0) and rh[0] == F(9.0) and o.n_rr == 1
    for bad in (np.nan, -1.0, 0.0):  # sqrt(NaN), sqrt(-1) and 0 > 0 all fail
        assert ck.cg_apply(0, ck.Block(itermax=9, eps=0.0, hist_cap=4), bad, np.zeros(4, F), None, 0)[0].stop == 1
    # eps is compared with the float the double root was stored to
    rr = F(2.0)
    root = F(np.sqrt(np.float64(rr)))
    assert ck.normr_fails(rr, root) == 1 and ck.normr_fails(rr, np.nextafter(root, F(0.0))) == 0
    # the fold kernels: vectors from the snapshot, the recorded step from the live fields
    r, p, x = np.array([1.0, 2.0], F), np.array([3.0, 5.0], F), np.array([0.5, 0.25], F)
    S = ck.Block(rr=3.0, snap_rr=7.0, iters=3, snap_iters=3, itermax=10, alpha=2.0, hist_cap=0)
    l1 = np.array([0.75, 0.25], F)
    o, pn, xn, _ = ck.update_p(1, S, r, p, x, 0, 2, l1)
    assert o.beta == np.float64(F(1.0) / F(3.0)) and same_bits(pn, r + (F(1.0) / F(7.0)) * p) and same_bits(xn, x + F(2.0) * p)
    o, pn, xn, _ = ck.update_p(1, S.copy(snap_stop_next=1), r, p, x, 0, 2, l1)
    assert pn is p and xn is x and o.iters == 4 and o.stop == 0  # (the live test passed, the snapshot's failed)
    o, pn, xn, _ = ck.update_p(1, S.copy(stop=1), r, p, x, 0, 2, l1)
    assert pn is p and xn is x and o is not None and np.array_equal(o.i(), S.copy(stop=1).i())
    o, pn, xn, _ = ck.update_p(0, S.copy(beta=0.5, x_pending=0), r, p, x, 0)
    assert same_bits(pn, r + F(0.5) * p) and xn is x
    o, rn, l1o, _, _ = ck.update_r(1, S.copy(neg_alpha=99.0), p, r, 2, l1, None, None)
    assert same_bits(rn, r + (-(F(3.0) / F(1.0))) * p) and len(l1o) == 1 and o.neg_alpha == F(-3.0)
    o, rn, l1o, _, _ = ck.update_r(0, S.copy(neg_alpha=-0.5, alpha=99.0), p, r)
    assert same_bits(rn, r + F(-0.5) * p) and o.alpha == F(99.0)


ENTRIES = {"sb_cg_update_p_native_f32": 12, "sb_cg_update_r_native_f32": 12, "sb_cg_scalar_native_f32": 12,
           "sb_cg_x_finalize_native_f32": 7, "sb_axpy_sdev_native_f32": 8, "sb_dot_l1_native_f32": 5, "sb_waxpby_stop_native_f32": 7,
           "sb_cg_update_p_launch_f32": 2, "sb_cg_update_r_launch_f32": 2, "sb_dot_l1_launch_f32": 2, "sb_stream_launch_f32": 2}


def test_entries_declared_exported_and_listed():
    """the blocking entries and launch queries: in include/sbhip.h, exported by the library, listed in capi with a prototype of
    as many parameters as the declaration; the control block is 7 floats, one double and 10 ints as the header says"""
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
    flat = " ".join(header.replace(" * ", " ").split())
    assert "blk_f[7] = {%s}" % ", ".join(ck.FIELDS_F) in flat
    assert "blk_i[10] = {%s}" % ", ".join(ck.FIELDS_I) in flat
    assert L.sb_is_initialized() == 0  # loading touched no device
