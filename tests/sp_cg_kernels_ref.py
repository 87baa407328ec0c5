"""The single-precision CG loop's vector and scalar kernels (kernels_sp.hip.h: cg_update_p_f32<0|1>, cg_update_r_f32<0|1>,
cg_scalar_f32_k<0|1|2>, cg_x_finalize_f32, axpy_sdev_f32_k, dot_l1_f32_k, waxpby_f32_k with a stop flag; kernels_sp_comm.hip.h:
cg_local_f32_k, cg_apply_local_f32_k<0|1|2>; pack_sp.hip.h: cg_x_finalize2_f32) restated on the CPU, one function per launch, in
numpy float32 on tests/sp_ref.py's `waxpby`, `level0`, `level1` and `level2`.  TEST INFRASTRUCTURE ONLY.

Per element one rounded float32 multiply and one rounded float32 add in the kernel's order; a level-1 value is
((q0 + q1) + q2) + q3 of its four level-0 partials; a total is sp_ref.level2 over the level-1 values.  `cg_apply` is the scalar
step (cg_apply_f32) as a function from control block to control block: the float quotient total / rr carried as a double,
alpha = rr / total and its negation, `normr_fails` (sqrt in double, stored to a float, !(normr > eps)), the histories' hist_cap
guard, defer_x and the snap_* copies.  Every launch function takes the block and the arrays as they are before the launch and
returns new ones: what a launch may not write comes back as the SAME object.  Which fields a launch reads is restated too:
cg_update_p_f32<1> takes its loop test from snap_iters / itermax / snap_stop_next and the vectors' beta from F(total / snap_rr),
while the recorder's step works on the whole block as it was (its beta, from rr, is what the block keeps);
cg_update_r_f32<1> forms -(rr / total) itself, cg_update_r_f32<0> reads neg_alpha.

tests/test_sp_cg_kernels_host.py pins these functions, chained in the loop's orders, to sp_ref.cg before anything on the GPU is
compared with them."""
import numpy as np

import sp_ref

F = np.float32
FIELDS_F = ("rr", "rr_old", "pAp", "alpha", "neg_alpha", "eps", "snap_rr")
FIELDS_I = ("stop", "stop_next", "iters", "n_rr", "n_pAp", "itermax", "hist_cap", "x_pending", "snap_iters", "snap_stop_next")


class Block:
    """the control block CgScalarsF: 7 floats, the double beta and 10 ints, in the order the test entries take them"""

    def __init__(self, **kw):
        for f in FIELDS_F:
            setattr(self, f, F(0.0))
        self.beta = np.float64(0.0)
        for f in FIELDS_I:
            setattr(self, f, 0)
        self.set(**kw)

    def set(self, **kw):
        for k, v in kw.items():
            assert k in FIELDS_F or k in FIELDS_I or k == "beta", k
            setattr(self, k, F(v) if k in FIELDS_F else np.float64(v) if k == "beta" else int(v))
        return self

    def copy(self, **kw):
        return Block(beta=self.beta, **{f: getattr(self, f) for f in FIELDS_F + FIELDS_I}).set(**kw)

    def f(self):
        return np.array([getattr(self, f) for f in FIELDS_F], dtype=F)

    def b(self):
        return np.array([self.beta], dtype=np.float64)

    def i(self):
        return np.array([getattr(self, f) for f in FIELDS_I], dtype=np.int32)

    @classmethod
    def from_arrays(cls, f, beta, i):
        b = cls()
        for name, v in zip(FIELDS_F, f):
            setattr(b, name, F(v))
        b.beta = np.float64(beta[0])
        for name, v in zip(FIELDS_I, i):
            setattr(b, name, int(v))
        return b

    def __repr__(self):
        return "Block(%s)" % ", ".join("%s=%r" % (f, getattr(self, f)) for f in FIELDS_F + ("beta",) + FIELDS_I)


def _f(a):
    return np.ascontiguousarray(a, dtype=F)


def groups(n):
    return (n + 255) // 256


def total_of(q, m, l1):
    """reduce_final_f32_1024(m, q, l1): q holds m level-1 values (l1) or 4 m level-0 partials"""
    q = _f(q) if q is not None else np.zeros(0, F)
    with np.errstate(all="ignore"):
        return F(sp_ref.level2(q[:m] if l1 else sp_ref.level1(q[:4 * m])))


def level1_of(a, b):
    """the ceil(n/256) level-1 values of a . b (dot_l1_f32_k, the tail of cg_update_r_f32)"""
    with np.errstate(all="ignore"):
        return sp_ref.level1(sp_ref.level0(a, b))


def normr_fails(rr, eps):
    with np.errstate(all="ignore"):
        return int(sp_ref.normr_fails(F(rr), F(eps)))


def axpy(x, a, y):
    """x + a y: the first branch of waxpby, whatever a is"""
    with np.errstate(all="ignore"):
        return _f(x) + F(a) * _f(y)


def _put(hist, at, v):
    hist = _f(hist).copy()
    hist[at] = v
    return hist


def cg_apply(mode, S, total, rr_hist, pAp_hist, defer_x):
    """cg_apply_f32<mode>(S, in = S, total, ...): the block and the two histories after the step (copies where written)"""
    total = F(total)
    o = S.copy()
    with np.errstate(all="ignore"):
        if mode == 0:
            sn = normr_fails(total, S.eps)
            o.rr, o.stop_next = total, sn
            if S.n_rr < S.hist_cap:
                rr_hist = _put(rr_hist, S.n_rr, total)
            o.n_rr = S.n_rr + 1
            if 1 < S.itermax and not sn:
                o.iters = 1
            else:
                o.stop = 1
        elif mode == 1:
            if S.iters + 1 < S.itermax and not S.stop_next:
                o.rr_old, o.rr = S.rr, total
                o.beta = np.float64(F(total / S.rr))  # the float division, carried by a double
                o.stop_next = normr_fails(total, S.eps)
                o.iters = S.iters + 1
                if S.n_rr < S.hist_cap:
                    rr_hist = _put(rr_hist, S.n_rr, total)
                o.n_rr = S.n_rr + 1
            else:
                o.stop = 1
            if defer_x:
                o.x_pending = 1
        else:
            o.x_pending = 0
            o.snap_rr, o.snap_iters, o.snap_stop_next = S.rr, S.iters, S.stop_next
            o.pAp = total
            al = F(S.rr / total)
            o.alpha, o.neg_alpha = al, F(-al)
            if S.n_pAp < S.hist_cap:
                pAp_hist = _put(pAp_hist, S.n_pAp, total)
            o.n_pAp = S.n_pAp + 1
    return o, rr_hist, pAp_hist


def update_p(mode, S, r, p, x, which, m=0, l1=None, rr_hist=None):
    """cg_update_p_f32<mode>: (S, p, x, rr_hist) after the launch.  mode 0 reads stop, beta (which == 0; the double narrowed to a
    float), x_pending and alpha and writes no field; mode 1 (which == 0) takes the loop test from snap_iters, itermax and
    snap_stop_next, beta from the total and snap_rr, alpha from the block, and the recorder takes cg_apply<1> with defer_x on
    the block as it was; a set stop flag writes nothing at all, a failed loop test only the block.  n = 0 in mode 1: the step
    alone (mode 0 is not launched then)"""
    with np.errstate(all="ignore"):
        if S.stop:  # (mode 1 reduces first and then looks at the flag: the same outcome)
            return S, p, x, rr_hist
        if mode == 0:
            beta = F(S.beta) if which == 0 else F(0.0)
            owed = x is not None and which == 0 and S.x_pending != 0
            out = S
        else:
            assert which == 0
            total = total_of(l1, m, 1)
            out, rr_hist, _ = cg_apply(1, S, total, rr_hist, None, 1)
            if not (S.snap_iters + 1 < S.itermax and not S.snap_stop_next):
                return out, p, x, rr_hist
            beta = F(total / S.snap_rr)
            owed = x is not None
        if len(r) == 0:
            return out, p, x, rr_hist
        b = p if which == 0 else r
        if owed:
            x = axpy(x, S.alpha, b)
        return out, axpy(r, beta, b), x, rr_hist


def update_r(mode, S, Ap, r, m=0, l1in=None, rr_hist=None, pAp_hist=None):
    """cg_update_r_f32<mode>: (S, r, l1out, rr_hist, pAp_hist) after the launch; l1out None: not written (stopped), else exactly
    ceil(n/256) values.  mode 0 reads stop and neg_alpha; mode 1 reads stop, rr and the m level-1 values, forms -(rr / total)
    itself, and the recorder takes cg_apply<2>"""
    with np.errstate(all="ignore"):
        if S.stop:
            return S, r, None, rr_hist, pAp_hist
        if mode == 0:
            nalpha, out = S.neg_alpha, S
        else:
            total = total_of(l1in, m, 1)
            nalpha = F(-F(S.rr / total))
            out, rr_hist, pAp_hist = cg_apply(2, S, total, rr_hist, pAp_hist, 0)
        if len(r) == 0:
            return out, r, np.zeros(0, F), rr_hist, pAp_hist
        rn = axpy(r, nalpha, Ap)
        return out, rn, level1_of(rn, rn), rr_hist, pAp_hist


def scalar(mode, S, q, m, defer_x, l1, rr_hist, pAp_hist):
    """cg_scalar_f32_k<mode>: (S, rr_hist, pAp_hist) after the launch"""
    if S.stop:
        return S, rr_hist, pAp_hist
    return cg_apply(mode, S, total_of(q, m, l1), rr_hist, pAp_hist, defer_x)


def local(S, q, m, l1, before):
    """cg_local_f32_k: what `local` holds after the launch (`before`, the same object, where the stop flag is set)"""
    return before if S.stop else total_of(q, m, l1)


def apply_local(mode, S, local_value, defer_x, rr_hist, pAp_hist):
    """cg_apply_local_f32_k<mode>: (S, rr_hist, pAp_hist) after the launch"""
    if S.stop:
        return S, rr_hist, pAp_hist
    return cg_apply(mode, S, F(local_value), rr_hist, pAp_hist, defer_x)


def x_finalize(S, x, p0, p1=None):
    """cg_x_finalize_f32 (p1 None) / cg_x_finalize2_f32: x after the launch (the block is read only)"""
    if not S.x_pending or len(x) == 0:
        return x
    return axpy(x, S.alpha, p0 if p1 is None or not S.n_pAp & 1 else p1)


def axpy_sdev(S, x, y, negative):
    """axpy_sdev_f32_k with the scalar at alpha / neg_alpha and the block's stop flag: w, or None where nothing is written"""
    if S.stop or len(x) == 0:
        return None
    return axpy(x, S.neg_alpha if negative else S.alpha, y)


def dot_l1(a, b, stopped):
    """dot_l1_f32_k: the ceil(n/256) level-1 values, or None where nothing is written"""
    if stopped or len(a) == 0:
        return None
    return level1_of(a, b)


def waxpby_stop(alpha, x, beta, y, stopped):
    """waxpby_f32_k with a stop pointer: w, or None where nothing is written"""
    if stopped or len(x) == 0:
        return None
    with np.errstate(all="ignore"):
        return sp_ref.waxpby(alpha, x, beta, y)
