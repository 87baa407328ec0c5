"""The double-precision CG loop's vector and scalar kernels (kernels.hip.h: cg_update_p<0|1|2>, cg_update_r_k<0|1|2>,
cg_scalar_k<MODE, REDUCE>, cg_x_finalize, dot_spans_k<1|2>, waxpby_sdev_k) restated on the CPU, one function per launch, on the
oracle's `waxpby`, `ddot_partials`, `reduce_final` and numpy.  TEST INFRASTRUCTURE ONLY: lives in tests/, the product never
imports the oracle.

Per element one rounded multiply and one rounded add in the kernel's order; a level-1 value is ((q0 + q1) + q2) + q3 of its four
level-0 partials; a total is the oracle's reduce_final over the level-1 values.  `cg_apply` is the scalar step as a function
from control block to control block, with the histories' hist_cap guard, defer_x and the snap_* copies.  Every launch function
takes the block and the arrays as they are before the launch and returns new ones: what a launch may not write comes back
as the SAME object, so a caller can tell "written with equal values" from "left alone" only on the GPU side, where it compares
bits and guards.  Which fields a launch reads is restated too: the fold kernels take their vector coefficients from snap_*, local
and alpha (BETA) / rr, local and stop (ALPHA), while the recorder's step works on the whole block as it was at the launch.

tests/test_cg_kernels_host.py pins these functions, chained in the loop's order, to the restatement of solveCG
(tests/cg_batch_ref.py) before anything on the GPU is compared with them."""
import numpy as np

from oracle import pyoracle as po

FIELDS_D = ("rr", "rr_old", "pAp", "alpha", "beta", "neg_alpha", "local", "eps", "snap_rr")
FIELDS_I = ("stop", "stop_next", "iters", "n_rr", "n_pAp", "itermax", "hist_cap", "x_pending", "p2p_error", "snap_iters",
            "snap_stop_next")


class Block:
    """the control block: 9 doubles and 11 ints in the order of the device's struct"""

    def __init__(self, **kw):
        for f in FIELDS_D:
            setattr(self, f, np.float64(0.0))
        for f in FIELDS_I:
            setattr(self, f, 0)
        self.set(**kw)

    def set(self, **kw):
        for k, v in kw.items():
            assert k in FIELDS_D or k in FIELDS_I, k
            setattr(self, k, np.float64(v) if k in FIELDS_D else int(v))
        return self

    def copy(self, **kw):
        return Block(**{f: getattr(self, f) for f in FIELDS_D + FIELDS_I}).set(**kw)

    def d(self):
        return np.array([getattr(self, f) for f in FIELDS_D], dtype=np.float64)

    def i(self):
        return np.array([getattr(self, f) for f in FIELDS_I], dtype=np.int32)

    @classmethod
    def from_arrays(cls, d, i):
        b = cls()
        for f, v in zip(FIELDS_D, d):
            setattr(b, f, np.float64(v))
        for f, v in zip(FIELDS_I, i):
            setattr(b, f, int(v))
        return b

    def __repr__(self):
        return "Block(%s)" % ", ".join("%s=%r" % (f, getattr(self, f)) for f in FIELDS_D + FIELDS_I)


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def groups(n):
    return (n + 255) // 256


def level0(x, y):
    """the 4 * ceil(n/256) level-0 partials of x . y: every aligned group of 64 elements as the xor butterfly adds it -- a
    balanced pairwise tree over the rounded products, missing elements +0.0"""
    x, y = _f(x), _f(y)
    n = len(x)
    with np.errstate(all="ignore"):
        v = np.zeros(4 * groups(n) * 64)
        v[:n] = x * y
        v = v.reshape(-1, 64)
        while v.shape[1] > 1:
            v = v[:, 0::2] + v[:, 1::2]
    return np.ascontiguousarray(v[:, 0])


def level1(q):
    """((q0 + q1) + q2) + q3 of every four level-0 partials"""
    q = _f(q).reshape(-1, 4)
    with np.errstate(all="ignore"):
        return ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]


def total_of(q, m, l1):
    """reduce_final_1024(m, q, l1): q holds m level-1 values (l1) or 4 m level-0 partials"""
    q = _f(q)
    with np.errstate(all="ignore"):
        return np.float64(po.reduce_final(q[:m] if l1 else level1(q[:4 * m])))


def cg_apply(mode, S, total, rr_hist, pAp_hist, defer_x):
    """cg_apply<mode>(S, in = S, total, ...): the block and the two histories after the step (copies where written)"""
    total = np.float64(total)
    o = S.copy()
    with np.errstate(all="ignore"):
        if mode == 0:
            sn = int(not (np.sqrt(total) > S.eps))
            o.rr, o.stop_next = total, sn
            if S.n_rr < S.hist_cap:
                rr_hist = _f(rr_hist).copy()
                rr_hist[S.n_rr] = total
            o.n_rr = S.n_rr + 1
            if 1 < S.itermax and not sn:
                o.iters = 1
            else:
                o.stop = 1
        elif mode == 1:
            if S.iters + 1 < S.itermax and not S.stop_next:
                o.rr_old, o.rr = S.rr, total
                o.beta = total / S.rr
                o.stop_next = int(not (np.sqrt(total) > S.eps))
                o.iters = S.iters + 1
                if S.n_rr < S.hist_cap:
                    rr_hist = _f(rr_hist).copy()
                    rr_hist[S.n_rr] = total
                o.n_rr = S.n_rr + 1
            else:
                o.stop = 1
            if defer_x:
                o.x_pending = 1
        else:
            o.x_pending = 0
            o.snap_rr, o.snap_iters, o.snap_stop_next = S.rr, S.iters, S.stop_next
            o.pAp = total
            al = S.rr / total
            o.alpha, o.neg_alpha = al, -al
            if S.n_pAp < S.hist_cap:
                pAp_hist = _f(pAp_hist).copy()
                pAp_hist[S.n_pAp] = total
            o.n_pAp = S.n_pAp + 1
    return o, rr_hist, pAp_hist


def update_p(mode, S, r, p, x, which, m=0, l1=None, rr_hist=None):
    """cg_update_p<mode>: (S, p, x, rr_hist) after the launch.  mode 0 reads stop, beta (which == 0), x_pending and alpha and
    writes no field; modes 1 / 2 (which == 0) take the loop test from snap_iters, itermax and snap_stop_next, beta from the
    total and snap_rr, alpha from the block, and the recorder takes cg_apply<1> on the block as it was; a set stop flag writes
    nothing at all, a failed loop test only the block"""
    with np.errstate(all="ignore"):
        if mode == 0:
            if S.stop:
                return S, p, x, rr_hist
            beta = float(S.beta) if which == 0 else 0.0
            owed = x is not None and which == 0 and S.x_pending != 0
            out = S
        else:
            assert which == 0
            if S.stop:  # (the kernel reduces first and then looks at the flag: the same outcome)
                return S, p, x, rr_hist
            total = total_of(l1, m, 1) if mode == 1 else S.local
            out, rr_hist, _ = cg_apply(1, S, total, rr_hist, None, 1)
            if not (S.snap_iters + 1 < S.itermax and not S.snap_stop_next):
                return out, p, x, rr_hist
            beta = float(np.float64(total) / S.snap_rr)
            owed = x is not None
        b = p if which == 0 else r
        if owed:
            x = po.waxpby(1.0, x, float(S.alpha), b)
        return out, po.waxpby(1.0, r, beta, b), x, rr_hist


def update_r(mode, S, Ap, r, m=0, l1in=None, rr_hist=None, pAp_hist=None):
    """cg_update_r_k<mode>: (S, r, l1out, rr_hist, pAp_hist) after the launch; l1out None: not written (stopped), else exactly
    ceil(n/256) values.  mode 0 reads stop and alpha (-alpha is formed here, neg_alpha is not read); modes 1 / 2 read stop, rr
    and the total (m level-1 values / local), and the recorder takes cg_apply<2>"""
    with np.errstate(all="ignore"):
        if mode == 0:
            if S.stop:
                return S, r, None, rr_hist, pAp_hist
            nalpha, out = -S.alpha, S
        else:
            if S.stop:
                return S, r, None, rr_hist, pAp_hist
            total = total_of(l1in, m, 1) if mode == 1 else S.local
            nalpha = -(S.rr / np.float64(total))
            out, rr_hist, pAp_hist = cg_apply(2, S, total, rr_hist, pAp_hist, 0)
        rn = po.waxpby(1.0, r, float(nalpha), Ap)
        return out, rn, po.ddot_partials(rn, rn), rr_hist, pAp_hist


def scalar(mode, reduce, S, q, m, to_local, defer_x, l1, rr_hist, pAp_hist):
    """cg_scalar_k<mode, reduce>: (S, rr_hist, pAp_hist) after the launch"""
    if S.stop:
        return S, rr_hist, pAp_hist
    total = total_of(q, m, l1) if reduce else S.local
    if reduce and to_local:
        return S.copy(local=total), rr_hist, pAp_hist
    return cg_apply(mode, S, total, rr_hist, pAp_hist, defer_x)


def x_finalize(S, x, p0, p1):
    """cg_x_finalize: x after the launch (the block is read only)"""
    if not S.x_pending:
        return x
    with np.errstate(all="ignore"):
        return po.waxpby(1.0, x, float(S.alpha), p1 if S.n_pAp & 1 else p0)


def dot_spans(op, S, a, b, x, r, stop=True):
    """dot_spans_k<op>: (x, r, partials) after the launch, partials None where the stop flag is set (stop: the launch was
    given the block's flag).  op 1: a = p, b = Ap; op 2: a = the right-hand side, b = Ap (alpha is not read)"""
    if stop and S.stop:
        return x, r, None
    with np.errstate(all="ignore"):
        if op == 1:
            x = po.waxpby(1.0, x, float(S.alpha), a)
            r = po.waxpby(1.0, r, float(-S.alpha), b)
        else:
            r = po.waxpby(1.0, a, -1.0, b)
        return x, r, level0(r, r)


def waxpby_sdev(S, x, y, negative):
    """waxpby_sdev_k with the scalar at alpha / neg_alpha and the block's stop flag: w, or None where nothing is written"""
    if S.stop:
        return None
    with np.errstate(all="ignore"):
        return po.waxpby(1.0, x, float(S.neg_alpha if negative else S.alpha), y)
