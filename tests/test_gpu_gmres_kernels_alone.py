"""Every kernel of the GMRES loop alone: gm_multidot_k, gm_finish_dots_k, gm_multiupdate_k<false, 2>, <false, 1>,
<true, 0>, gm_pre_multiupdate_k<0|1>, gm_scale_k / gm_pre_scale_k<0|1>, gm_rr_k<0|1|2>, gm_step_k<false>, <true>,
gm_pre_step_k<0|1> and gm_backsolve_k through the blocking entries that launch them with the loop's own launch functions, each ==
its CPU restatement (tests/gmres_kernels_ref.py, pinned by tests/test_gmres_kernels_host.py) BIT FOR BIT: NaN equal to NaN, -0.0
apart from +0.0, no tolerance.  The control block and the dense state go in and come out as plain data and are compared whole.

Every output sits between sentinels and starts as the sentinel; every input that is not an output is compared with its upload;
the padding of V behind n is NaN; a stopped call leaves every output equal to its sentinel.  Vectors come from specials(): NaN,
+-Inf, -0.0 and subnormals at distinct positions of distinct vectors.

Sizes: the small ones around the lane, the pair, the two-element tail, the 256-row group and the partial odd group, and the sizes
at which a wave / a thread of the capped grid takes a second trip, from the launches the library reports (sb_gmres_group_launch,
sb_gmres_scale_launch, sb_gmres_step_launch) and printed, never written down here."""
import numpy as np
import pytest

from oracle import pyoracle as po

import gmres_kernels_ref as gk
from sparsebench_amd.capi import DeviceVector
from test_gpu_bicgstab_kernels import SENTINEL, Guarded, same, specials
from test_gpu_gmres_kernels import second_trip_n
from test_gpu_gmres_precond_kernels import finite_specials

pytestmark = pytest.mark.gpu

SMALL = [1, 2, 63, 64, 129, 255, 256, 257, 511, 513, 1430, 4099]
NVECS = [1, 3, 4, 5, 8]  # below, at and past MD_UNROLL
C1 = 0.7853981633974483  # a Chebyshev c1 with a full mantissa
GROUP_KINDS = ["dot", "epi2", "epi1", "add", "pre0", "pre1"]
MODE = {"add": -1, "pre0": 0, "pre1": 1}


def query(L, name, n):
    out = np.zeros(3, dtype=np.uint32)
    getattr(L, name)(n, out.ctypes.data)
    return int(out[0]), int(out[1]), int(out[2])


@pytest.fixture(scope="module")
def big(gpu):
    """the second-trip sizes, from the launch queries"""
    s = {"group": second_trip_n(gpu)}
    cap, threads, cus = query(gpu, "sb_gmres_scale_launch", 0x7FFFFF00)
    assert threads == 256 and cap >= cus >= 1
    s["scale"] = cap * 256 + 3
    assert query(gpu, "sb_gmres_scale_launch", s["scale"])[0] == cap and query(gpu, "sb_gmres_scale_launch", 257)[0] == 2
    cap, threads, cus = query(gpu, "sb_gmres_step_launch", 0x7FFFFF00)
    assert threads == 1024 and cap == cus
    s["step"] = cus * 4096 + 4099
    assert query(gpu, "sb_gmres_step_launch", s["step"])[0] == cus
    assert query(gpu, "sb_gmres_step_launch", 4099)[0] == 2 and query(gpu, "sb_gmres_step_launch", 1)[0] == 1
    print("second-trip sizes on %d CUs:" % cus, s)
    return s


def all_sentinel(buf, what):
    assert np.all(buf.get(what) == SENTINEL), (what, "written")


def free(*bufs):
    for b in bufs:
        if b is not None:
            b.free()


def ptr(b):
    return b.ptr if b is not None else None


def same_block(got, want, what):
    same(got.d(), want.d(), what + ("control block", gk.FIELDS_D))
    assert np.array_equal(got.i(), want.i()), (what, "control block", [(f, int(a), int(b)) for f, a, b in zip(gk.FIELDS_I, got.i(), want.i()) if a != b])


def same_dense(got, want, what):
    for name in gk.DENSE:
        same(getattr(got, name), getattr(want, name), what + ("dense state", name))


# ---- the group kernels ----------------------------------------------------------------------------------------------------------
class Basis:
    """nvec vectors of n rows on the device, vector i at i * ldv, NaN behind n (never read: it must not show)"""

    def __init__(self, V):
        self.V = V
        self.nvec, self.n = V.shape
        self.ldv = ((self.n + 1) // 2) * 2 + 6
        host = np.full((self.nvec, self.ldv), np.nan)
        host[:, :self.n] = V
        self.dv = DeviceVector.from_host(host.reshape(-1))
        self.ptr = self.dv.ptr

    def kept(self, what):
        same(self.dv.get().reshape(self.nvec, self.ldv)[:, :self.n], self.V, what + ("V untouched",))

    def free(self):
        self.dv.free()


def clean_last_group(vs, n, seed):
    """finite non-zero values in the last 256-row group of every vector: with an infinite coefficient every row of the group
    is +-Inf and no NaN hides what the rows behind n add"""
    rng = np.random.default_rng(seed)
    lo = 256 * ((n - 1) // 256)
    for v in vs:
        v[lo:] = rng.uniform(0.5, 2.0, n - lo) * rng.choice([-1.0, 1.0], n - lo)


def run_group(L, kind, B, w, c, dinv, stopped, what):
    """one launch of a group kernel on the basis B against its restatement"""
    n, nvec, nG = B.n, B.nvec, gk.groups(B.n)
    what = (kind, n, nvec, "stopped" if stopped else "") + tuple(what)
    V = list(B.V)
    dw, dc = Guarded(w), Guarded(c)
    dl = dd = d_d = d_z = None
    if kind == "dot":
        dl = Guarded(n=nvec * nG)
        rc = L.sb_gmres_multidot_native(n, nvec, B.ptr, B.ldv, dw.ptr, dl.ptr, stopped)
        want_w, want_l1 = w, gk.multidot(V, w, stopped)
    elif kind in ("epi1", "epi2"):
        epi = int(kind[-1])
        dl = Guarded(n=nvec * nG if epi == 2 else nG)
        rc = L.sb_gmres_project_native(epi, n, nvec, B.ptr, B.ldv, dc.ptr, dw.ptr, dl.ptr, stopped)
        want_w, want_l1 = gk.project(epi, V, c, w, stopped)
    else:
        mode = MODE[kind]
        if mode >= 0:
            dd, d_d, d_z = Guarded(dinv), Guarded(n=n), Guarded(n=n)
        rc = L.sb_gmres_multiadd_native(n, mode, C1, nvec, B.ptr, B.ldv, dc.ptr, dw.ptr, ptr(dd), ptr(d_d), ptr(d_z), stopped)
        want_w, want_d, want_z = gk.multiadd(mode, C1, V, c, w, dinv, stopped)
        for buf, want, name in ((d_d, want_d, "d"), (d_z, want_z, "z")):
            if buf is not None and want is None:
                all_sentinel(buf, what + (name,))
            elif buf is not None:
                same(buf.get(name), want, what + (name,))
    assert rc == 0, (what, "guard words around the stop flag changed", rc)
    same(dw.get("w"), want_w, what + ("w",))
    if dl is not None and want_l1 is None:
        all_sentinel(dl, what + ("l1",))
    elif dl is not None:
        same(dl.get("l1"), want_l1, what + ("l1",))
    same(dc.get("c"), c, what + ("c untouched",))
    if dd is not None:
        same(dd.get("dinv"), dinv, what + ("dinv untouched",))
    B.kept(what)
    free(dw, dc, dl, dd, d_d, d_z)


@pytest.mark.parametrize("kind", GROUP_KINDS)
@pytest.mark.parametrize("n", SMALL)
def test_group_kernels_at_the_small_sizes(gpu, n, kind):
    for nvec in NVECS:
        vs = specials(n, 3000 + 10 * n + nvec, nvec + 2)
        B = Basis(np.stack(vs[:nvec]))
        w, dinv = vs[nvec], vs[nvec + 1]
        c = np.random.default_rng(n + nvec).standard_normal(nvec)
        run_group(gpu, kind, B, w, c, dinv, 0, ())
        if nvec == 5:
            run_group(gpu, kind, B, w, c, dinv, 1, ())
        B.free()
        # finite inputs: no NaN in any group, so every level-1 value is compared as a number
        fs = [finite_specials(n, 3500 + 100 * n + 10 * nvec + i) for i in range(nvec + 2)]
        B = Basis(np.stack(fs[:nvec]))
        run_group(gpu, kind, B, fs[nvec], c, fs[nvec + 1], 0, ("finite",))
        B.free()


@pytest.mark.parametrize("kind", GROUP_KINDS[1:])
@pytest.mark.parametrize("n", [n for n in SMALL if n % 256])
def test_group_kernels_with_special_coefficients_in_a_partial_group(gpu, n, kind):
    """c[0] = +Inf, c[nvec-1] = NaN, c = -0.0: rows behind n are loaded as +0.0, and 0.0 - Inf * 0.0 is NaN -- the epilogues force
    them back to +0.0 before their dots.  The last group's own rows are finite and non-zero, so that its level-1 values are +-Inf
    under c[0] = +Inf and a NaN from behind n shows"""
    for nvec in (1, 3, 4, 5):
        vs = specials(n, 4000 + 10 * n + nvec, nvec + 2)
        clean_last_group(vs, n, n + nvec)
        B = Basis(np.stack(vs[:nvec]))
        w, dinv = vs[nvec], vs[nvec + 1]
        base = np.random.default_rng(2 * n + nvec).standard_normal(nvec)
        for name in ("inf_first", "nan_last", "minus_zero"):
            c = base.copy()
            if name == "inf_first":
                c[0] = np.inf
            elif name == "nan_last":
                c[nvec - 1] = np.nan
            else:
                c[:] = -0.0
            run_group(gpu, kind, B, w, c, dinv, 0, (name,))
        if kind in ("epi1", "epi2"):  # the case itself: the last group's values are infinite, not NaN
            c = base.copy()
            c[0] = np.inf
            l1 = gk.project(int(kind[-1]), list(B.V), c, w)[1]
            assert np.isinf(l1[gk.groups(n) - 1]), (n, nvec, l1)
        B.free()


@pytest.fixture(scope="module")
def big_inputs(gpu, big):
    """(basis, w, dinv) at the second-trip size per (nvec, finite), made once and kept on the device for the six kernels that read
    them; freed when the module is done, whichever tests ran"""
    made = {}

    def get(nvec, finite):
        if (nvec, finite) not in made:
            n = big["group"]
            vs = [finite_specials(n, 5100 + 10 * nvec + i) for i in range(nvec + 2)] if finite else specials(n, 5000 + nvec, nvec + 2)
            made[(nvec, finite)] = (Basis(np.stack(vs[:nvec])), vs[nvec], vs[nvec + 1])
        return made[(nvec, finite)]

    yield get
    for B, _, _ in made.values():
        B.free()


@pytest.mark.parametrize("kind", GROUP_KINDS)
@pytest.mark.parametrize("nvec", [1, 5])
def test_group_kernels_on_a_second_trip(gpu, big, big_inputs, nvec, kind):
    """one full group more than the capped grid has waves, then a partial odd one: both are a wave's second group.  Once with the
    special values, once with finite inputs, where the second trip's level-1 values are compared as numbers"""
    n = big["group"]
    print("second grid-stride trip with a partial last group at n =", n)
    c = np.random.default_rng(nvec).standard_normal(nvec)
    for finite in (0, 1):
        B, w, dinv = big_inputs(nvec, finite)
        run_group(gpu, kind, B, w, c, dinv, 0, ("finite",) if finite else ())


# ---- gm_finish_dots_k -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l1", [1, 0])
@pytest.mark.parametrize("nGroups", [1, 15, 16, 17, 1024, 1025])
@pytest.mark.parametrize("nvec", [1, 5, 31])
def test_finish_dots(gpu, nvec, nGroups, l1):
    per = nGroups if l1 else 4 * nGroups
    stride = per + 6 + (per & 1)  # larger than what a workgroup reads, and even
    rng = np.random.default_rng(100 * nvec + nGroups + l1)
    q = np.full(nvec * stride, np.nan)  # what lies between two dots' values is never read: NaN there must not show
    for i in range(nvec):
        q[i * stride:i * stride + per] = rng.standard_normal(per) * 10.0 ** rng.integers(-3, 4, per)
    add = rng.standard_normal(nvec)
    if nvec > 1:  # sums of zeros of either sign, an infinite value and a NaN in dots of their own
        q[1 * stride:1 * stride + per] = 0.0
        q[2 * stride:2 * stride + per] = -0.0
        q[3 * stride + per // 2] = np.inf
        q[4 * stride + per - 1] = np.nan
        add[1], add[2] = -0.0, -0.0
    else:
        q[:per] = -0.0 if nGroups == 15 else q[:per]
    dq, da = Guarded(q), Guarded(add)
    for with_nout, with_sum, stopped in ((1, 1, 0), (0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1)):
        what = ("finish_dots", nvec, nGroups, l1, with_nout, with_sum, stopped)
        want = gk.finish_dots(nGroups, q, stride, l1, nvec, add if with_sum else None, stopped)
        d_out, d_nout, d_sum = Guarded(n=nvec), Guarded(n=nvec), Guarded(n=nvec)
        rc = gpu.sb_gmres_finish_dots_native(nGroups, nvec, dq.ptr, stride, l1, d_out.ptr, d_nout.ptr if with_nout else None,
                                             da.ptr if with_sum else None, d_sum.ptr if with_sum else None, stopped)
        assert rc == 0, what
        if stopped:
            for b in (d_out, d_nout, d_sum):
                all_sentinel(b, what)
        else:
            same(d_out.get("out"), want[0], what + ("out",))
            if with_nout:
                same(d_nout.get("nout"), want[1], what + ("nout = -out, the sign of a zero included",))
            else:
                all_sentinel(d_nout, what + ("nout",))
            if with_sum:
                same(d_sum.get("sum"), want[2], what + ("sum = add + out",))
            else:
                all_sentinel(d_sum, what + ("sum",))
        free(d_out, d_nout, d_sum)
    same(dq.get("q"), q, ("q untouched",)), same(da.get("add"), add, ("add untouched",))
    free(dq, da)


# ---- gm_rr_k --------------------------------------------------------------------------------------------------------------------
def rr_block(**kw):
    base = dict(normr=0.75, eps=1.0, hn=1.25, rr=3.5, stop=0, k=7, j=3, itermax=50, n_res=7, n_rr=2, hist_cap=6, cycles=1, steps=6)
    base.update(kw)
    return gk.Block(**base)


# name -> (block fields, the values r.r is reduced from (their sum is exact), use_stop); sqrt(4.0) = 2.0 against eps
RR_SCENARIOS = {
    "plain": (dict(), [1.0, 2.5, 0.5], 1),
    "history_empty": (dict(n_rr=0, n_res=0), [4.0], 1),
    "history_last_slot": (dict(n_rr=5), [4.0], 1),
    "history_full": (dict(n_rr=6), [4.0], 1),
    "hist_cap_0": (dict(hist_cap=0, n_rr=0), [4.0], 1),
    "itermax_1": (dict(itermax=1, k=1), [4.0], 1),
    "k_is_itermax_minus_1": (dict(itermax=8), [4.0], 1),
    "k_is_itermax": (dict(itermax=7), [4.0], 1),
    "norm_below_eps": (dict(eps=3.0), [4.0], 1),
    "norm_equals_eps": (dict(eps=2.0), [4.0], 1),
    "norm_above_eps": (dict(eps=1.0), [4.0], 1),
    "rr_zero": (dict(eps=0.0), [0.0, 0.0], 1),
    "rr_nan": (dict(), [1.0, np.nan], 1),
    "rr_inf": (dict(), [np.inf, 1.0], 1),
    "stopped": (dict(stop=1), [4.0], 1),
    "stopped_without_a_flag": (dict(stop=1), [4.0], 0),
    "no_flag": (dict(), [4.0], 0),
}


@pytest.mark.parametrize("name", list(RR_SCENARIOS))
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_rr(gpu, mode, name):
    kw, values, use_stop = RR_SCENARIOS[name]
    S = rr_block(**kw)
    cap = max(S.hist_cap, 1)
    for l1 in (1, 0):
        nG = len(values)
        q = np.array(values) if l1 else np.array([[v, 0.0, 0.0, 0.0] for v in values]).reshape(-1)
        res, rrh = np.full(cap, SENTINEL), np.full(cap, SENTINEL)
        want_S, want_res, want_rr = gk.rr(mode, S, q, nG, l1, res, rrh, use_stop)
        dq, d_res, d_rr = Guarded(q), Guarded(res), Guarded(rrh)
        d, i = S.d(), S.i()
        rc = gpu.sb_gmres_rr_native(mode, nG, dq.ptr, l1, d_res.ptr, d_rr.ptr, use_stop, d.ctypes.data, i.ctypes.data)
        what = ("gm_rr_k", mode, name, "l1", l1)
        assert rc == 0, (what, "guard words around the control block changed", rc)
        same_block(gk.Block.from_arrays(d, i), want_S, what)
        same(d_res.get("res_hist"), want_res, what + ("res_hist",))
        same(d_rr.get("rr_hist"), want_rr, what + ("rr_hist",))
        same(dq.get("q"), q, what + ("q untouched",))
        if name == "stopped":
            assert want_S is S and want_res is res and want_rr is rrh
        if mode == 2:  # the close sb_gmres_finish makes never touches normr or stop
            assert d[0] == S.normr and i[0] == S.stop
        free(dq, d_res, d_rr)


# ---- the scalar step ------------------------------------------------------------------------------------------------------------
M_STEP = 6
STEP_KINDS = {"step_false": (0, -1), "step_true": (1, -1), "pre_step_0": (1, 0), "pre_step_1": (1, 1)}


def arnoldi_states():
    """the dense state in front of every step launch of one real cycle of the restatement (48 rows, restart length 6)"""
    n, m = 48, M_STEP
    rng = np.random.default_rng(48)
    A = rng.standard_normal((n, n)) + 4.0 * np.eye(n)
    r = rng.standard_normal(n)
    nG = gk.groups(n)
    S = gk.Block(k=1, itermax=50, eps=1e-12, hist_cap=20, n_res=1, n_rr=1)
    S.normr = np.sqrt(np.float64(po.ddot_tree(r, r)))
    D, res = gk.Dense(m), np.full(20, SENTINEL)
    v0, g0, _, _ = gk.scale(-1, 0.0, r, S.normr)
    D.g[0] = g0
    V, out = [v0], []
    for j in range(m):
        nvec = j + 1
        w = A @ V[j]
        D.h1[:nvec], D.nh1[:nvec], _ = gk.finish_dots(nG, gk.multidot(V, w), nG, 1, nvec)
        w, l1 = gk.project(2, V, D.h1[:nvec], w)
        D.h2[:nvec], D.nh2[:nvec], D.hcol[:nvec] = gk.finish_dots(nG, l1, nG, 1, nvec, D.h1)
        w, l1 = gk.project(1, V, D.h2[:nvec], w)
        out.append(D.copy())
        S, D, res, v, _, _ = gk.step(True, -1, 0.0, S, D, j, l1, nG, 1, w, None, res)
        V.append(v)
    assert S.stop == 0 and all(np.all(np.isfinite(d.pack())) for d in out) and abs(out[-1].cs[4]) > 0.0 and abs(out[-1].sn[4]) > 0.0
    return out


def hand_set_state(m):
    """distinct values everywhere (another column, another cs, sn, g or y entry that changes shows); exact rotations"""
    D = gk.Dense(m, 1.0 + np.arange(m * (m + 1) + 3 * m + 6 * (m + 1)) / 64.0)
    rot = [(0.6, 0.8), (-0.8, 0.6), (0.28, -0.96), (1.0, 0.0), (0.0, 1.0), (-0.6, -0.8)]
    for i in range(m):
        D.cs[i], D.sn[i] = rot[i % len(rot)]
    D.hcol[:] = [(-1.0) ** i * (0.75 + i / 8.0) for i in range(m + 1)]
    return D


@pytest.fixture(scope="module")
def states():
    return dict(arnoldi=arnoldi_states(), hand=hand_set_state(M_STEP))


def step_block(j, **kw):
    base = dict(normr=0.75, eps=1e-12, hn=1.25, rr=3.5, stop=0, k=7, j=j, itermax=50, n_res=7, n_rr=2, hist_cap=20, cycles=1, steps=6)
    base.update(kw)
    return gk.Block(**base)


def run_step(L, kind, S, D, j, w, dinv, what, l1_form=1):
    """one launch of a step kernel against its restatement; returns the restatement's block"""
    scale, mode = STEP_KINDS[kind]
    n, nG = len(w), gk.groups(len(w))
    with np.errstate(all="ignore"):
        q = po.ddot_partials(w, w) if l1_form else gk.level0(w, w)
    res = np.full(max(S.hist_cap, 1), SENTINEL)
    want_S, want_D, want_res, want_v, want_d, want_z = gk.step(bool(scale), mode, C1, S, D, j, q, nG, l1_form, w, dinv, res)
    dq, dw, d_res = Guarded(q), Guarded(w), Guarded(res)
    dd = Guarded(dinv) if mode >= 0 else None
    d_v, d_d, d_z = Guarded(n=n), Guarded(n=n), Guarded(n=n)
    d, i, dense = S.d(), S.i(), D.pack()
    rc = L.sb_gmres_step_native(scale, mode, C1, n, j, D.m, nG, dq.ptr, l1_form, dw.ptr, d_v.ptr, ptr(dd), d_d.ptr if mode >= 0 else None,
                                d_z.ptr if mode >= 0 else None, d_res.ptr, d.ctypes.data, i.ctypes.data, dense.ctypes.data)
    assert rc == 0, (what, "guard words around the state changed", rc)
    same_block(gk.Block.from_arrays(d, i), want_S, what)
    same_dense(gk.Dense(D.m, dense), want_D, what)
    same(d_res.get("res_hist"), want_res, what + ("res_hist",))
    raised = want_S.stop and not S.stop
    for buf, want, name in ((d_v, want_v, "vnext"), (d_d, want_d, "d"), (d_z, want_z, "z")):
        got = buf.get(name)
        if want is None:
            assert np.all(got == SENTINEL), (what, name, "written")
        elif raised:  # a late workgroup may already see the flag this step raises: V[j+1] may be incomplete, never wrong
            a, b = np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64)
            ok = (got == SENTINEL) | (a == b) | (np.isnan(got) & np.isnan(want))
            assert np.all(ok), (what, name, "neither the sentinel nor the value at", np.nonzero(~ok)[0][:5])
        else:
            same(got, want, what + (name,))
    same(dq.get("q"), q, what + ("q untouched",)), same(dw.get("w"), w, what + ("w untouched",))
    if dd is not None:
        same(dd.get("dinv"), dinv, what + ("dinv untouched",))
    free(dq, dw, d_res, dd, d_v, d_d, d_z)
    return want_S, want_D


STEP_SCENARIOS = ["plain", "history_last_slot", "history_full", "hist_cap_0", "last_step", "norm_equals_eps", "hn_zero", "hn_nan",
                  "hjj_zero", "stopped"]


@pytest.mark.parametrize("rot", ["arnoldi", "hand"])
@pytest.mark.parametrize("j", [0, 1, 4, M_STEP - 1])
@pytest.mark.parametrize("kind", list(STEP_KINDS))
def test_scalar_step_scenarios(gpu, states, kind, j, rot):
    n = 1430
    D0 = states["arnoldi"][j] if rot == "arnoldi" else states["hand"]
    dinv = specials(n, 6000 + j, 1)[0]
    w0 = finite_specials(n, 6100 + j)
    for name in STEP_SCENARIOS:
        what = (kind, "j", j, rot, name)
        S, D, w = step_block(j), D0, w0
        if name == "history_last_slot":
            S = step_block(j, hist_cap=8)
        elif name == "history_full":
            S = step_block(j, hist_cap=7)
        elif name == "hist_cap_0":
            S = step_block(j, hist_cap=0)
        elif name == "last_step":  # k + 1 == itermax
            S = step_block(j, itermax=8)
        elif name == "norm_equals_eps":
            S = step_block(j, eps=abs(run_step(gpu, kind, S, D, j, w, dinv, what + ("to take the estimate",))[0].normr))
        elif name == "hn_zero":  # d = |hjj|, s = 0; eps < 0 keeps the loop going on an estimate of 0
            S, w = step_block(j, eps=-1.0), np.where(np.arange(n) % 2, -0.0, 0.0)
        elif name == "hn_nan":
            w = w0.copy()
            w[n // 3] = np.nan
        elif name == "hjj_zero":
            D = D0.copy()
            D.hcol[:] = 0.0
        elif name == "stopped":
            S = step_block(j, stop=1)
        want_S, want_D = run_step(gpu, kind, S, D, j, w, dinv, what, l1_form=0 if kind == "step_false" and name == "plain" else 1)
        if name == "stopped":
            assert want_S is S and want_D is D
        elif name == "norm_equals_eps":
            assert want_S.stop == 1 and want_S.normr == S.eps
        elif name == "last_step" or name == "hn_nan":
            assert want_S.stop == 1
        elif name == "hn_zero":
            assert want_S.stop == 0 and want_D.sn[j] == 0.0 and want_D.h(j, j) == abs(want_D.h(j, j)) and want_S.normr == 0.0
        elif name == "plain":
            assert want_S.stop == 0 and (rot != "arnoldi" or j == 0 or want_D.h(0, j) != D.hcol[0])  # earlier rotations bite


@pytest.mark.parametrize("kind", list(STEP_KINDS)[1:])
@pytest.mark.parametrize("n", SMALL + ["capped"])
def test_step_and_normalise_at_every_size(gpu, big, states, kind, n):
    """V[j+1] and the riders: n = 4 099 is a third trip on a 2-workgroup grid, CUs * 4096 + 4099 one on the capped grid"""
    n = big["step"] if n == "capped" else n
    dinv, w_sp = specials(n, 7000 + n % 1000, 2)
    for j, w in ((1, finite_specials(n, 7100 + n % 1000)), (4, finite_specials(n, 7200 + n % 1000)), (4, w_sp)):
        assert run_step(gpu, kind, step_block(j), states["hand"], j, w, dinv, (kind, n, "j", j))[0].stop == int(w is w_sp)
    run_step(gpu, kind, step_block(1, stop=1), states["hand"], 1, w_sp, dinv, (kind, n, "stopped"))


# ---- gm_backsolve_k -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 5, 30])
def test_backsolve(gpu, m):
    D0 = gk.Dense(m, (1.0 + np.arange(m * (m + 1) + 3 * m + 6 * (m + 1)) / 128.0) * np.where(np.arange(m * (m + 1) + 3 * m + 6 * (m + 1)) % 3, 1.0, -1.0))
    assert len(set(D0.H.tolist())) == len(D0.H)  # distinct everywhere: a transposed or mis-strided read shows
    for nvec in sorted({1, m - 1, m} - {0}):
        for name in ("plain", "zero_diagonal", "stopped", "stopped_without_a_flag"):
            D = D0.copy()
            S = step_block(nvec, stop=int(name.startswith("stopped")))
            use_stop = int(name != "stopped_without_a_flag")
            if name == "zero_diagonal":  # +-Inf or NaN flows through the rows above
                D.H[(nvec - 1) * (m + 1) + nvec - 1] = 0.0
            want = gk.backsolve(S, D, nvec, use_stop)
            d, i, dense = S.d(), S.i(), D.pack()
            rc = gpu.sb_gmres_backsolve_native(m, nvec, use_stop, d.ctypes.data, i.ctypes.data, dense.ctypes.data)
            what = ("gm_backsolve_k", m, nvec, name)
            assert rc == 0, what
            same_block(gk.Block.from_arrays(d, i), S, what)
            got = gk.Dense(m, dense)
            same_dense(got, want, what)
            same(got.y[nvec:], D.y[nvec:], what + ("y behind nvec",))
            if name == "stopped":
                assert want is D
            else:
                assert not np.array_equal(got.y[:nvec], D.y[:nvec]), what
            if name == "zero_diagonal":
                assert not np.isfinite(got.y[nvec - 1])


# ---- gm_scale_k, gm_pre_scale_k -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [-1, 0, 1])
@pytest.mark.parametrize("n", [1, 257, 4099, "second_trip"])
def test_scale(gpu, big, n, mode):
    """cap * 256 + 3 rows: three threads of the capped grid take a second row"""
    n = big["scale"] if n == "second_trip" else n
    a, dinv = specials(n, 8000 + n % 1000, 2)
    da, dd = Guarded(a), Guarded(dinv) if mode >= 0 else None
    for scalar, with_g0, stopped in ((1.7109375, 1, 0), (-3.0e-5, 0, 0), (1.7109375, 1, 1)):
        what = ("scale", n, mode, scalar, with_g0, stopped)
        want_out, want_g0, want_d, want_z = gk.scale(mode, C1, a, scalar, dinv, stopped)
        ds = DeviceVector.from_host(np.array([scalar, SENTINEL]))
        dg, d_out, d_d, d_z = Guarded(n=1), Guarded(n=n), Guarded(n=n), Guarded(n=n)
        rc = gpu.sb_gmres_scale_native(n, mode, C1, da.ptr, ds.ptr, d_out.ptr, dg.ptr if with_g0 else None, ptr(dd),
                                       d_d.ptr if mode >= 0 else None, d_z.ptr if mode >= 0 else None, stopped)
        assert rc == 0, what
        for buf, want, name in ((d_out, want_out, "out"), (d_d, want_d, "d"), (d_z, want_z, "z"), (dg, [want_g0] if with_g0 and not stopped else None, "g0")):
            if want is None:
                all_sentinel(buf, what + (name,))
            else:
                same(buf.get(name), want, what + (name,))
        assert np.array_equal(ds.get(), [scalar, SENTINEL])
        free(ds, dg, d_out, d_d, d_z)
    same(da.get("a"), a, ("a untouched",))
    if dd is not None:
        same(dd.get("dinv"), dinv, ("dinv untouched",))
    free(da, dd)
