"""The kernels of restarted GMRES(m) (gmres.hip.h: gm_multidot_k, gm_finish_dots_k, gm_multiupdate_k<ADD, EPI>, gm_scale_k,
gm_rr_k<0|1|2>, gm_step_k<SCALE>, gm_backsolve_k and the three gm_pre_* twins) restated on the CPU, one function per launch, on
the oracle's `ddot_partials`, `ddot_tree`, `reduce_final`, `waxpby`, on gmres_ref's `_sqrt` / `_div` and numpy.  TEST
INFRASTRUCTURE ONLY: lives in tests/, the product never imports the oracle.

Every product is rounded before its add or subtract; a level-1 value is the oracle's ddot_partials entry of its 256-row group
(missing rows +0.0); a total is reduce_final over the level-1 values (or over ((q0 + q1) + q2) + q3 of level-0 partials).  The
scalar steps are loops on Python floats, every operation rounded on its own, in the kernels' order.  Every launch function takes
the block, the dense state and the vectors as they are before the launch and returns new ones: what a launch may not write comes
back as the SAME object (arrays) or as None (output-only arrays), so the GPU tests compare "left alone" with bits and sentinels.
The stop flag is honoured where the kernel honours it: `stopped` stands for the flag a launch is handed (`use_stop`: the block's
own, or none), and gm_step_k reads the block's flag itself.

tests/test_gmres_kernels_host.py pins these functions, chained in the loop's order, to gmres_ref.solve."""
import math

import numpy as np

from oracle import pyoracle as po

import gmres_precond_ref
from cg_kernels_ref import groups, level0, level1, total_of  # (the tree dot's levels, shared with the CG loop's restatement)
from gmres_ref import _div, _sqrt

FIELDS_D = ("normr", "eps", "hn", "rr")
FIELDS_I = ("stop", "k", "j", "itermax", "n_res", "n_rr", "hist_cap", "cycles", "steps")
DENSE = ("H", "cs", "sn", "y", "g", "h1", "h2", "nh1", "nh2", "hcol")  # the order gm_dense_layout gives them


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class Block:
    """the control block (GmScalars): 4 doubles and 9 ints in the order of the device's struct"""

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
        return cls(**dict(zip(FIELDS_D, d)), **dict(zip(FIELDS_I, i)))

    def __repr__(self):
        return "Block(%s)" % ", ".join("%s=%r" % (f, getattr(self, f)) for f in FIELDS_D + FIELDS_I)


def dense_sizes(m):
    return dict(H=m * (m + 1), cs=m, sn=m, y=m, g=m + 1, h1=m + 1, h2=m + 1, nh1=m + 1, nh2=m + 1, hcol=m + 1)


class Dense:
    """the dense state of a cycle of restart length m: H column-major with leading dimension m + 1 (H[i][j] at H[j * (m + 1)
    + i]), then cs, sn, y (m each) and g, h1, h2, nh1, nh2, hcol (m + 1 each) -- one flat array on the device"""

    def __init__(self, m, flat=None):
        self.m = m
        sizes = dense_sizes(m)
        total = sum(sizes.values())
        assert total == m * (m + 1) + 3 * m + 6 * (m + 1)
        flat = np.zeros(total) if flat is None else _f(flat).copy()
        assert flat.shape == (total,)
        o = 0
        for name in DENSE:
            setattr(self, name, flat[o:o + sizes[name]].copy())
            o += sizes[name]

    def pack(self):
        return np.concatenate([getattr(self, name) for name in DENSE])

    def copy(self):
        return Dense(self.m, self.pack())

    def h(self, i, j):
        return self.H[j * (self.m + 1) + i]


# ---- the vector kernels ---------------------------------------------------------------------------------------------------------
def multidot(V, w, stopped=0):
    """gm_multidot_k: l1[i * nGroups + g] = level-1 value of dot(V[i], w) in group g; None: stopped, nothing written"""
    if stopped:
        return None
    w = _f(w)
    with np.errstate(all="ignore"):
        return np.concatenate([po.ddot_partials(_f(v), w) for v in V])


def finish_dots(nGroups, q, qStride, l1, nvec, add=None, stopped=0):
    """gm_finish_dots_k on nvec workgroups: (out, nout, sum) of nvec entries each (sum None without add); None: stopped"""
    if stopped:
        return None
    q = _f(q)
    per = nGroups if l1 else 4 * nGroups
    with np.errstate(all="ignore"):
        out = np.array([total_of(q[i * qStride:i * qStride + per], nGroups, l1) for i in range(nvec)])
        return out, -out, None if add is None else _f(add)[:nvec] + out


def _combine(V, c, w, sign):
    w = np.array(w, dtype=np.float64)
    with np.errstate(all="ignore"):
        for v, ci in zip(V, c):
            t = np.float64(ci) * _f(v)
            w = w - t if sign < 0 else w + t
    return w


def project(epi, V, c, w, stopped=0):
    """gm_multiupdate_k<false, epi>: (w, l1) after the launch; epi 0: l1 None; 1: the ceil(n/256) level-1 values of w . w;
    2: those of dot(V[i], w) against the UPDATED w at l1[i * nGroups + g]; (w, None) with w the same object: stopped"""
    if stopped:
        return w, None
    wn = _combine(V, c, w, -1)
    with np.errstate(all="ignore"):
        if epi == 1:
            return wn, po.ddot_partials(wn, wn)
        if epi == 2:
            return wn, multidot(V, wn)
    return wn, None


def rider(mode, c1, v, dinv):
    """what rides in a producer of v: (d, z); mode -1 nothing, 0 a diagonal (z only), 1 Chebyshev (d = z)"""
    if mode < 0:
        return None, None
    f = gmres_precond_ref.first(v, dinv, c1 if mode else None)
    return (f if mode else None), f


def multiadd(mode, c1, V, c, w, dinv=None, stopped=0):
    """gm_multiupdate_k<true, 0> (mode -1) / gm_pre_multiupdate_k<mode>: (w, d, z) after the launch"""
    if stopped:
        return w, None, None
    wn = _combine(V, c, w, +1)
    return (wn,) + rider(mode, c1, wn, dinv)


def scale(mode, c1, a, scalar, dinv=None, stopped=0):
    """gm_scale_k (mode -1) / gm_pre_scale_k<mode>: (out, g0, d, z) after the launch; g0 = the scalar"""
    if stopped:
        return None, None, None, None
    with np.errstate(all="ignore"):
        out = _f(a) / np.float64(scalar)
    return (out, np.float64(scalar)) + rider(mode, c1, out, dinv)


# ---- the scalar kernels ---------------------------------------------------------------------------------------------------------
def _put(hist, at, v):
    hist = _f(hist).copy()
    hist[at] = v
    return hist


def rr(mode, S, q, nGroups, l1, res_hist, rr_hist, use_stop=0):
    """gm_rr_k<mode>: (S, res_hist, rr_hist) after the launch.  MODE 0 the prologue, 1 a close inside the loop, 2 the close of
    sb_gmres_finish, which never touches normr or stop"""
    if use_stop and S.stop:
        return S, res_hist, rr_hist
    total = float(total_of(q, nGroups, l1))
    o = S.copy(rr=total, n_rr=S.n_rr + 1)
    if S.n_rr < S.hist_cap:
        rr_hist = _put(rr_hist, S.n_rr, total)
    if mode == 0:
        normr = _sqrt(total)
        o.set(normr=normr, n_res=1, k=1, j=0)
        if 0 < S.hist_cap:
            res_hist = _put(res_hist, 0, normr)
        if not (1 < S.itermax and normr > float(S.eps)):
            o.stop = 1
    else:
        o.set(cycles=S.cycles + 1, j=0)
        if mode == 1:
            normr = _sqrt(total)
            o.normr = np.float64(normr)
            if not (S.k < S.itermax and normr > float(S.eps)):
                o.stop = 1
    return o, res_hist, rr_hist


def scalar_step(S, D, j, hn, res_hist):
    """gm_scalar_step: (S, D, res_hist) after the scalar step at cycle position j with hn = ||w||"""
    m = D.m
    assert 0 <= j < m
    o, E = S.copy(), D.copy()
    ld = m + 1
    Hj = [float(v) for v in D.hcol[:j + 1]] + [float(v) for v in D.H[j * ld + j + 1:(j + 1) * ld]]
    hn = float(hn)
    for i in range(j):
        ci, si, a, b = float(D.cs[i]), float(D.sn[i]), Hj[i], Hj[i + 1]
        t = ci * a + si * b
        Hj[i + 1] = ci * b - si * a
        Hj[i] = t
    hjj = Hj[j]
    d = _sqrt(hjj * hjj + hn * hn)
    c, s = _div(hjj, d), _div(hn, d)
    Hj[j] = d
    E.H[j * ld:(j + 1) * ld] = Hj
    E.cs[j], E.sn[j] = c, s
    gj = float(D.g[j])
    gn = -(s * gj)
    E.g[j + 1] = gn
    E.g[j] = c * gj
    normr = math.fabs(gn)
    o.set(normr=normr, hn=hn, n_res=S.k + 1, k=S.k + 1, j=j + 1, steps=S.steps + 1)
    if S.k < S.hist_cap:
        res_hist = _put(res_hist, S.k, normr)
    if not (S.k + 1 < S.itermax and normr > float(S.eps)):
        o.stop = 1
    return o, E, res_hist


def step(scale_too, mode, c1, S, D, j, q, nGroups, l1, w=None, dinv=None, res_hist=None):
    """gm_step_k<scale_too> (mode -1) / gm_pre_step_k<mode>: (S, D, res_hist, vnext, d, z) after the launch.  The kernel reads the
    block's own stop flag: a block that arrives stopped changes nothing.  scale_too: vnext = w / hn and its rider (a launch that
    raises the flag may leave them incomplete on the device; here they are whole)"""
    if S.stop:
        return S, D, res_hist, None, None, None
    hn = _sqrt(total_of(q, nGroups, l1))
    o, E, res_hist = scalar_step(S, D, j, hn, res_hist)
    if not scale_too:
        return o, E, res_hist, None, None, None
    with np.errstate(all="ignore"):
        v = _f(w) / np.float64(hn)
    return (o, E, res_hist, v) + rider(mode, c1, v, dinv)


def backsolve(S, D, nvec, use_stop=0):
    """gm_backsolve_k: D after the launch (only y[0 .. nvec-1] changes)"""
    if (use_stop and S.stop) or nvec == 0:
        return D
    E = D.copy()
    y = [float(v) for v in D.y]
    for i in range(nvec - 1, -1, -1):
        t = float(D.g[i])
        for l in range(i + 1, nvec):
            t = t - float(D.h(i, l)) * y[l]
        y[i] = _div(t, float(D.h(i, i)))
    E.y[:] = y
    return E
