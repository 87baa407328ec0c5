"""The double-precision CG loop's vector and scalar kernels alone: cg_update_p<0|1|2>, cg_update_r_k<0|1|2>,
cg_scalar_k<MODE, REDUCE>, cg_x_finalize, dot_spans_k<1|2> and waxpby_sdev_k through the blocking entries that launch them with
the loop's own launch functions, each == its CPU restatement (tests/cg_kernels_ref.py, pinned by tests/test_cg_kernels_host.py)
BIT FOR BIT: NaN equal to NaN, -0.0 apart from +0.0, no tolerance.  The control block goes in and comes out as plain data and
is compared field by field.

Every device array sits between guards of quiet NaNs with a payload (512 doubles behind its logical end) that are compared as
bits after the launch; what a launch may not write -- its inputs, and everything on a set stop flag or a failed loop test -- is
compared with its upload as bits; output slots (level-1 values, partials, histories) start as a payload NaN, so "exactly
ceil(n/256) written" is literal.

Sizes: n = 1 .. 4 097 around the lane, span and group edges, and the sizes at which a thread / a wave of the capped grid takes a
second trip, derived from the launches the library reports (sb_cg_update_p_launch, sb_cg_update_r_launch) and printed, never
written down here.  Every vector comes in a finite variant (+0.0, -0.0, denormals at the first and last element and at the
256-group boundary) and a special one (+-inf and a NaN there as well)."""
import numpy as np
import pytest

import cg_kernels_ref as ck
import precond_ref
from sparsebench_amd.capi import DeviceVector
from test_gpu_sgs_kernels import same

pytestmark = pytest.mark.gpu

GUARD, FRONT = 512, 64
GUARD_BITS = 0x7FF8C0DE00000000
FILL_BITS = np.uint64(0x7FF8F111F111F111)
SMALL = [1, 2, 3, 127, 128, 129, 255, 256, 257, 511, 513, 4097]
P_SIZES = ["p_stride-1", "p_stride", "p_stride+1", "p_2stride", "p_2stride+1", "p_3stride+5_odd"]
R_SIZES = ["r_one_trip", "r_one_group_more", "r_two_trips_257", "r_one_trip_1"]
BIG = ["p_3stride+5_odd", "r0_two_trips_257"]
ALPHA, BETA, LOCAL = 0.8046875, -1.2890625, 2.71875  # exactly representable
MAX_N = 5 << 20


def fill(n):
    return np.full(n, FILL_BITS, dtype=np.uint64).view(np.float64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Buf:
    """n doubles on the device, 64 guard doubles in front and 512 behind; data None: n payload-NaN slots"""

    def __init__(self, data=None, n=None):
        self.n = len(data) if data is not None else n
        up = np.uint64(GUARD_BITS) + np.arange(FRONT + self.n + GUARD, dtype=np.uint64)
        up[FRONT:FRONT + self.n] = bits(data) if data is not None else FILL_BITS
        self.up = up
        self.dv = DeviceVector.from_host(up.view(np.float64))
        self.ptr = self.dv.ptr + 8 * FRONT

    def get(self, what):
        a = self.dv.get().view(np.uint64)
        lo, hi = FRONT, FRONT + self.n
        front, back = np.nonzero(a[:lo] != self.up[:lo])[0], np.nonzero(a[hi:] != self.up[hi:])[0]
        assert front.size == 0, (what, "guard in front overwritten at element", int(front[0]) - lo)
        assert back.size == 0, (what, "guard behind overwritten at element", self.n + int(back[0]))
        return a[lo:hi].copy().view(np.float64)

    def kept(self, what):
        """payload and guards as uploaded, bit for bit"""
        got = bits(self.get(what))
        bad = np.nonzero(got != self.up[FRONT:FRONT + self.n])[0]
        assert bad.size == 0, (what, "changed at", int(bad[0]), "of", bad.size)

    def check(self, want, orig, what):
        """want is orig (the restatement's 'not written'): the upload's bits; else the restatement's values"""
        if want is orig:
            return self.kept(what + ("not to be written",))
        same(self.get(what), want, what)

    def slots(self, want, what):
        """an output array of slots: the restatement's values where it wrote, the untouched payload NaN elsewhere"""
        got = self.get(what)
        same(got, want, what)
        gw, ww = bits(got) == FILL_BITS, bits(want) == FILL_BITS
        assert np.array_equal(gw, ww), (what, "written slots differ at", np.nonzero(gw != ww)[0][:5], "of", len(got))

    def free(self):
        self.dv.free()


def free(*bufs):
    for b in bufs:
        if b is not None:
            b.free()


def ptr(b):
    return b.ptr if b is not None else None


_base = {}


def vecs(n, special):
    """r, p, x, Ap of n rows: slices of four vectors made once (precond_ref.probe_vector: mixed sign and magnitude), with the
    edge values at the first element, the last, both sides of the 256-group boundary, n/2 and n/3 -- another kind in each vector"""
    tiny = 5e-324 * 1000
    kinds = [0.0, -0.0, tiny, np.inf, -np.inf, np.nan] if special else [0.0, -0.0, tiny, -tiny, 1e-310, -0.0]
    out = []
    for w in range(4):
        if w not in _base:
            _base[w] = precond_ref.probe_vector(MAX_N, 11 + w, False)
        v = _base[w][:n].copy()
        for j, pos in enumerate([0, n - 1, 255, 256, n // 2, n // 3]):
            if pos < n:
                v[pos] = kinds[(j + w) % 6]
        out.append(v)
    return out


def launch_p(L, n):
    out = np.zeros(3, dtype=np.uint32)
    L.sb_cg_update_p_launch(n, out.ctypes.data)
    return int(out[0]), int(out[1]), int(out[2])


def launch_r(L, n, mode):
    out = np.zeros(3, dtype=np.uint32)
    L.sb_cg_update_r_launch(n, mode, out.ctypes.data)
    return int(out[0]), int(out[1]), int(out[2])


@pytest.fixture(scope="module")
def sizes(gpu):
    """name -> n.  cg_update_p: thread t of W x T takes the double2 t and t + stride, then refills at t + 2 stride; cg_update_r_k
    <mode>: a wave per 256-row group, 16 W waves in mode's own grid"""
    s = {k: k for k in SMALL}
    W, T, cus = launch_p(gpu, 0x7FFFFF00)
    assert T == 1024 and W >= cus >= 1
    stride = W * T
    for name, n2, odd in zip(P_SIZES, (stride - 1, stride, stride + 1, 2 * stride, 2 * stride + 1, 3 * stride + 5), (0, 0, 0, 0, 0, 1)):
        s[name] = 2 * n2 + odd
        assert launch_p(gpu, s[name])[0] == W, name
    assert launch_p(gpu, 1)[0] == 1 and launch_p(gpu, 4097)[0] == min(W, 3)
    print("cg_update_p: %d workgroups x %d threads on %d CUs;" % (W, T, cus), {k: s[k] for k in P_SIZES})
    for mode in (0, 1, 2):
        W, T, _ = launch_r(gpu, 0x7FFFFF00, mode)
        assert T == 1024
        waves = W * (T // 64)
        for name, n in zip(R_SIZES, (256 * waves, 256 * (waves + 1), 256 * 2 * waves + 257, 256 * waves + 1)):
            key = "r%d_%s" % (mode, name[2:])
            s[key] = n
            assert launch_r(gpu, n, mode)[0] == W, key
        assert launch_r(gpu, 1, mode)[0] == 1 and launch_r(gpu, 4097, mode)[0] == min(W, 2)
        print("cg_update_r_k<%d>: %d workgroups, %d waves;" % (mode, W, waves), {k: v for k, v in s.items() if str(k).startswith("r%d_" % mode)})
    assert launch_r(gpu, 0x7FFFFF00, 1)[0] <= launch_r(gpu, 0x7FFFFF00, 0)[0] == launch_r(gpu, 0x7FFFFF00, 2)[0]
    assert max(s.values()) <= MAX_N
    return s


def same_block(got, want, what):
    same(got.d(), want.d(), what + ("control block", ck.FIELDS_D))
    assert np.array_equal(got.i(), want.i()), (what, "control block", [(f, int(a), int(b)) for f, a, b in zip(ck.FIELDS_I, got.i(), want.i()) if a != b])


def block(**kw):
    """a block of a running loop whose live rr / iters differ from their snapshot twins"""
    base = dict(rr=3.5, rr_old=9.25, pAp=11.5, alpha=ALPHA, beta=BETA, neg_alpha=-ALPHA, local=LOCAL, eps=1e-9, snap_rr=1.75, stop=0, stop_next=0,
                iters=7, n_rr=2, n_pAp=3, itermax=50, hist_cap=6, x_pending=0, p2p_error=0, snap_iters=4, snap_stop_next=0)
    base.update(kw)
    return ck.Block(**base)


def level1_values(m, seed, zero=False):
    """m positive level-1 values of mixed magnitude"""
    rng = np.random.RandomState(seed)
    return np.zeros(m) if zero else rng.random_sample(m) * 10.0 ** rng.randint(-3, 4, size=m) + 2.0 ** -20


# ---- cg_update_p ---------------------------------------------------------------------------------------------------------------
def run_update_p(L, mode, S, r, p, x, which, m=0, l1=None, hist=None, what=()):
    what = ("cg_update_p", mode, len(r), "which", which) + tuple(what)
    want_S, want_p, want_x, want_h = ck.update_p(mode, S, r, p, x, which, m, l1, hist)
    dr, dp, dx = Buf(r), Buf(p), Buf(x) if x is not None else None
    dl, dh = Buf(l1) if l1 is not None else None, Buf(hist) if hist is not None else None
    d, i = S.d(), S.i()
    rc = L.sb_cg_update_p_native(mode, len(r), dr.ptr, dp.ptr, ptr(dx), which, m, ptr(dl), ptr(dh), d.ctypes.data, i.ctypes.data)
    assert rc == 0, (what, "guard words around the control block changed", rc)
    same_block(ck.Block.from_arrays(d, i), want_S, what)
    dp.check(want_p, p, what + ("p",))
    if dx:
        dx.check(want_x, x, what + ("x",))
    dr.kept(what + ("r",))
    if dl:
        dl.kept(what + ("level-1 values",))
    if dh:
        dh.slots(want_h, what + ("rr history",))
    free(dr, dp, dx, dl, dh)
    return want_S, want_p, want_x


@pytest.mark.parametrize("xcase", ["no_x", "x_not_pending", "x_pending"])
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("size", SMALL + P_SIZES)
def test_update_p_without_a_step(gpu, sizes, size, which, xcase):
    """cg_update_p<0>: which = 1 is the literal r + 0.0 r (an infinite r gives NaN, -0.0 stays -0.0) and touches no x; the owed
    x update is taken on the OLD p, only with x and the pending flag; the block is not written"""
    n = sizes[size]
    for special in (False, True):
        r, p, x, _ = vecs(n, special)
        S = block(x_pending=int(xcase == "x_pending"))
        xin = None if xcase == "no_x" else x
        _, wp, wx = run_update_p(gpu, 0, S, r, p, xin, which, what=(xcase, special))
        if which == 1:
            neg0 = bits(r) == bits(np.array([-0.0]))[0]
            assert np.all(bits(wp)[neg0] == bits(np.array([-0.0]))[0]) and np.all(np.isnan(wp[np.isinf(r)]))
        assert (wx is not xin) == (xcase == "x_pending" and which == 0)


@pytest.mark.parametrize("size", [3, 257, 4097, "p_2stride+1"])
def test_update_p_stopped_changes_nothing(gpu, sizes, size):
    n = sizes[size]
    r, p, x, _ = vecs(n, True)
    for mode in (0, 1, 2):
        for which in (0, 1) if mode == 0 else (0,):
            l1, hist = (level1_values(5, 1), fill(6)) if mode else (None, None)
            _, wp, wx = run_update_p(gpu, mode, block(stop=1, x_pending=1), r, p, x, which, 5 if mode else 0, l1, hist, what=("stopped",))
            assert wp is p and wx is x


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("size", SMALL + P_SIZES)
def test_update_p_with_the_beta_step(gpu, sizes, size, mode):
    """cg_update_p<1|2> at every size: the loop test passes, beta = total / snap_rr, the x update is owed; with x and without"""
    n = sizes[size]
    m = 37
    for special in (False, True):
        r, p, x, _ = vecs(n, special)
        _, wp, wx = run_update_p(gpu, mode, block(), r, p, x if not special else None, 0, m, level1_values(m, n % 97), fill(6), what=(special,))
        assert wp is not p and (special or wx is not x)


FOLD_P = {
    "passes": {},
    "fails_on_itermax": dict(itermax=5),                                  # snap_iters + 1 == itermax (and the live test fails too)
    "fails_on_itermax_in_the_snapshot_only": dict(itermax=9, snap_iters=8),  # live: 7 + 1 < 9
    "passes_in_the_snapshot_only": dict(itermax=6),                       # live: 7 + 1 < 6 fails, the snapshot's 4 + 1 < 6 passes
    "fails_on_snap_stop_next": dict(snap_stop_next=1, stop_next=1),
    "fails_on_snap_stop_next_in_the_snapshot_only": dict(snap_stop_next=1),
    "stop_next_live_only": dict(stop_next=1),
    "stopped": dict(stop=1),
    "history_full": dict(n_rr=6),
    "history_of_no_entries": dict(n_rr=0, hist_cap=0),
    "x_pending_already": dict(x_pending=1),
    "converges": dict(eps=1e30),
    "snap_rr_zero": dict(snap_rr=0.0),
    "total_nan": dict(local=np.nan),
}


@pytest.mark.parametrize("scenario", list(FOLD_P))
@pytest.mark.parametrize("mode", [1, 2])
def test_update_p_beta_step_scenarios(gpu, mode, scenario):
    """the loop test from the SNAPSHOT (snap_iters, snap_stop_next), beta from snap_rr -- the live rr / iters / stop_next differ
    from them, as they do for a late workgroup once the recorder has stored the step; the recorded step from the block as it
    was.  A set stop flag writes nothing, a failed test the block alone; at n_rr == hist_cap no history store, n_rr advances"""
    kw = dict(FOLD_P[scenario])
    m = 5
    l1 = level1_values(m, 3)
    if scenario == "total_nan" and mode == 1:
        l1[2] = np.nan
    for n in (2, 513):
        r, p, x, _ = vecs(n, False)
        S = block(**kw)
        cap = S.hist_cap
        wS, wp, wx = run_update_p(gpu, mode, S, r, p, x, 0, m, l1, fill(cap), what=(scenario,))
        if scenario in ("passes", "history_full", "passes_in_the_snapshot_only", "stop_next_live_only"):
            assert wp is not p and wx is not x
        if scenario.startswith("fails") or scenario == "stopped":
            assert wp is p and wx is x
        if scenario == "history_full":
            assert wS.n_rr == 7
        if scenario == "stopped":
            assert wS is S


@pytest.mark.parametrize("m", [1, 1024, 1025, 8193])
def test_update_p_total_of_m_level1_values(gpu, m):
    """cg_update_p<1>: every workgroup reduces the m level-1 values itself; 8 193 reaches the 8-wide unrolled part"""
    for n in (129, 4097):
        r, p, x, _ = vecs(n, False)
        wS, wp, _ = run_update_p(gpu, 1, block(), r, p, x, 0, m, level1_values(m, m), fill(6), what=("m", m))
        assert wS.rr == ck.total_of(level1_values(m, m), m, 1) and wp is not p


@pytest.mark.parametrize("coeff", [np.inf, -np.inf, np.nan, 0.0, -0.0])
def test_update_p_special_coefficients(gpu, coeff):
    for n in (257, 513):
        for special in (False, True):
            r, p, x, _ = vecs(n, special)
            run_update_p(gpu, 0, block(beta=coeff, x_pending=1), r, p, x, 0, what=("beta", coeff))
            run_update_p(gpu, 0, block(alpha=coeff, x_pending=1), r, p, x, 0, what=("alpha", coeff))
            run_update_p(gpu, 2, block(alpha=coeff, local=coeff), r, p, x, 0, 0, None, fill(6), what=("alpha and total", coeff))


# ---- cg_update_r_k -------------------------------------------------------------------------------------------------------------
def run_update_r(L, mode, S, Ap, r, m=0, l1in=None, rr_hist=None, pAp_hist=None, what=()):
    n = len(r)
    what = ("cg_update_r_k", mode, n) + tuple(what)
    want_S, want_r, want_l1, want_rh, want_ph = ck.update_r(mode, S, Ap, r, m, l1in, rr_hist, pAp_hist)
    dA, dr, do = Buf(Ap), Buf(r), Buf(n=ck.groups(n))
    dl = Buf(l1in) if l1in is not None else None
    drh, dph = Buf(rr_hist) if rr_hist is not None else None, Buf(pAp_hist) if pAp_hist is not None else None
    d, i = S.d(), S.i()
    rc = L.sb_cg_update_r_native(mode, n, dA.ptr, dr.ptr, do.ptr, m, ptr(dl), ptr(drh), ptr(dph), d.ctypes.data, i.ctypes.data)
    assert rc == 0, (what, "guard words around the control block changed", rc)
    same_block(ck.Block.from_arrays(d, i), want_S, what)
    dr.check(want_r, r, what + ("r",))
    dA.kept(what + ("Ap",))
    if want_l1 is None:
        do.kept(what + ("level-1 values of a stopped launch",))
    else:
        assert len(want_l1) == ck.groups(n)
        do.slots(want_l1, what + ("level-1 values",))
        assert not np.any(bits(do.get(what)) == FILL_BITS), (what, "a level-1 slot below ceil(n/256) was not written")
    if dl:
        dl.kept(what + ("level-1 input",))
    if drh:
        drh.slots(want_rh, what + ("rr history",))
    if dph:
        dph.slots(want_ph, what + ("pAp history",))
    free(dA, dr, do, dl, drh, dph)
    return want_S, want_r, want_l1


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("size", SMALL + R_SIZES)
def test_update_r(gpu, sizes, size, mode):
    """r += -alpha Ap and the level-1 values of r.r: exactly ceil(n/256) slots; modes 1 / 2 against the restated cg_apply<2>
    (alpha, neg_alpha, pAp, the pAp history, n_pAp, x_pending cleared, the snapshot copies), in each mode's own grid"""
    n = sizes[size if size in SMALL else "r%d_%s" % (mode, size[2:])]
    m = 41
    for special in (False, True):
        r, _, _, Ap = vecs(n, special)
        if mode == 0:
            run_update_r(gpu, 0, block(), Ap, r, what=(special,))
        else:
            wS, _, _ = run_update_r(gpu, mode, block(x_pending=1), Ap, r, m, level1_values(m, n % 89), fill(6), fill(6), what=(special,))
            assert (wS.snap_rr, wS.snap_iters, wS.snap_stop_next, wS.x_pending, wS.n_pAp) == (3.5, 7, 0, 0, 4)


FOLD_R = {
    "passes": {},
    "stopped": dict(stop=1),
    "history_full": dict(n_pAp=6),
    "history_of_no_entries": dict(n_pAp=0, hist_cap=0),
    "stop_next_is_copied": dict(stop_next=1),
    "total_zero": dict(local=0.0),          # alpha = rr / 0 = +inf
    "total_zero_rr_zero": dict(local=0.0, rr=0.0),  # alpha = NaN
    "total_negative_zero": dict(local=-0.0),
    "total_nan": dict(local=np.nan),
}


@pytest.mark.parametrize("scenario", list(FOLD_R))
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_update_r_alpha_step_scenarios(gpu, mode, scenario):
    kw = dict(FOLD_R[scenario])
    m = 5
    l1 = level1_values(m, 4, zero=scenario.startswith("total_zero") or scenario == "total_negative_zero")
    if scenario == "total_nan":
        l1[4] = np.nan
    if mode == 0:  # the coefficient is the block's alpha: the one the scenario's total would have given
        kw["alpha"] = {"total_zero": np.inf, "total_zero_rr_zero": np.nan, "total_negative_zero": -np.inf, "total_nan": np.nan}.get(scenario, ALPHA)
    for n in (2, 513):
        for special in (False, True):
            r, _, _, Ap = vecs(n, special)
            S = block(**kw)
            hists = (fill(S.hist_cap), fill(S.hist_cap)) if mode else (None, None)
            with np.errstate(all="ignore"):
                wS, wr, wl = run_update_r(gpu, mode, S, Ap, r, m if mode else 0, l1 if mode else None, *hists, what=(scenario, special))
            if scenario == "stopped":
                assert wS is S and wr is r and wl is None
            elif mode and scenario == "history_full":
                assert wS.n_pAp == 7
            elif mode and scenario == "total_zero":
                assert wS.alpha == np.inf and wS.neg_alpha == -np.inf and not np.isfinite(wr).any()
            elif mode and scenario == "total_zero_rr_zero":
                assert np.isnan(wS.alpha) and np.isnan(wr).all()


@pytest.mark.parametrize("m", [1, 1024, 1025, 8193])
def test_update_r_total_of_m_level1_values(gpu, m):
    for n in (129, 4097):
        r, _, _, Ap = vecs(n, False)
        wS, _, _ = run_update_r(gpu, 1, block(), Ap, r, m, level1_values(m, m + 1), fill(6), fill(6), what=("m", m))
        assert wS.pAp == ck.total_of(level1_values(m, m + 1), m, 1)


# ---- cg_scalar_k ---------------------------------------------------------------------------------------------------------------
def run_scalar(L, mode, reduce, S, q, m, to_local, defer_x, l1, cap, what=()):
    what = ("cg_scalar_k", mode, bool(reduce), "m", m, "to_local", to_local, "defer_x", defer_x, "l1", l1) + tuple(what)
    rh, ph = fill(cap), fill(cap)
    want_S, want_rh, want_ph = ck.scalar(mode, reduce, S, q, m, to_local, defer_x, l1, rh, ph)
    dq, drh, dph = Buf(q), Buf(rh), Buf(ph)
    d, i = S.d(), S.i()
    rc = L.sb_cg_scalar_native(mode, int(reduce), m, dq.ptr, drh.ptr, dph.ptr, to_local, defer_x, l1, d.ctypes.data, i.ctypes.data)
    assert rc == 0, (what, "guard words around the control block changed", rc)
    same_block(ck.Block.from_arrays(d, i), want_S, what)
    dq.kept(what + ("q",))
    drh.slots(want_rh, what + ("rr history",))
    dph.slots(want_ph, what + ("pAp history",))
    free(dq, drh, dph)
    return want_S


ROOT2 = float(np.sqrt(np.float64(2.0)))
SCALAR = {
    "runs": {},
    "stopped": dict(stop=1),
    "history_full": dict(n_rr=6, n_pAp=6),
    "history_of_no_entries": dict(n_rr=0, n_pAp=0, hist_cap=0),
    "itermax_1": dict(itermax=1, iters=0),
    "itermax_2": dict(itermax=2, iters=0),
    "last_body": dict(itermax=9),
    "stop_next_set": dict(stop_next=1),
    "total_zero": dict(local=0.0),
    "total_nan": dict(local=np.nan),
    "eps_equals_the_norm": dict(local=2.0, eps=ROOT2),
    "eps_one_ulp_below_the_norm": dict(local=2.0, eps=float(np.nextafter(ROOT2, 0.0))),
    "eps_one_ulp_above_the_norm": dict(local=2.0, eps=float(np.nextafter(ROOT2, 4.0))),
}


@pytest.mark.parametrize("scenario", list(SCALAR))
@pytest.mark.parametrize("reduce", [1, 0])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_scalar_step(gpu, mode, reduce, scenario):
    """every MODE x REDUCE the library launches: the step on the total (reduce: of q, as one level-1 value or four level-0
    partials; else `local`), to_local, defer_x, l1 0 and 1; sqrt(total) > eps decided by one ulp"""
    S = block(**SCALAR[scenario])
    total = float(S.local)
    with np.errstate(all="ignore"):
        for l1, defer_x in ((1, 0), (1, 1), (0, 0), (0, 1)) if reduce else ((0, 0), (0, 1)):
            q = np.array([total, 0.0, 0.0, 0.0] if not l1 else [total, 0.0])
            if reduce:
                S = S.copy(local=-77.0)  # (not read)
            wS = run_scalar(gpu, mode, reduce, S, q, 1, 0, defer_x, l1, S.hist_cap, what=(scenario,))
            if scenario.startswith("eps") and mode < 2:
                assert wS.stop_next == int(scenario != "eps_one_ulp_below_the_norm")
            if scenario == "itermax_1" and mode == 0:
                assert wS.stop == 1 and wS.iters == 0
            if scenario == "stopped":
                assert wS is S
        if reduce:
            wS = run_scalar(gpu, mode, 1, S, np.array([total, 0.0]), 1, 1, 1, 1, S.hist_cap, what=(scenario, "to_local"))
            assert np.array_equal(wS.i(), S.i()) and (scenario in ("stopped", "total_nan") or wS.local == total)


@pytest.mark.parametrize("m", [1, 3, 1024, 1025, 8193])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_scalar_step_reduces_m_values(gpu, mode, m):
    for l1 in (1, 0):
        q = level1_values(m if l1 else 4 * m, 7 * m + l1)
        for to_local in (0, 1):
            wS = run_scalar(gpu, mode, 1, block(), q, m, to_local, 1, l1, 6, what=("reduction",))
            assert (wS.local if to_local else (wS.pAp if mode == 2 else wS.rr)) == ck.total_of(q, m, l1)


# ---- cg_x_finalize -------------------------------------------------------------------------------------------------------------
def run_x_finalize(L, S, x, p0, p1, what=()):
    what = ("cg_x_finalize", len(x)) + tuple(what)
    want = ck.x_finalize(S, x, p0, p1)
    dx, d0, d1 = Buf(x), Buf(p0), Buf(p1)
    d, i = S.d(), S.i()
    rc = L.sb_cg_x_finalize_native(len(x), dx.ptr, d0.ptr, d1.ptr, d.ctypes.data, i.ctypes.data)
    assert rc == 0, (what, "guard words around the control block changed", rc)
    same_block(ck.Block.from_arrays(d, i), S, what)
    dx.check(want, x, what + ("x",))
    d0.kept(what + ("p0",)), d1.kept(what + ("p1",))
    free(dx, d0, d1)
    return want


@pytest.mark.parametrize("size", SMALL + BIG)
def test_x_finalize(gpu, sizes, size):
    """x += alpha p of the buffer n_pAp names (odd: p1), only where the update is pending; the two buffers hold different data"""
    n = sizes[size]
    for special in (False, True):
        _, p0, x, p1 = vecs(n, special)
        for n_pAp in (4, 7, 0, 1) if n <= 4097 else (4, 7) if not special else (7,):
            want = run_x_finalize(gpu, block(x_pending=1, n_pAp=n_pAp), x, p0, p1, what=(special, n_pAp))
            with np.errstate(all="ignore"):
                same(want, x + ALPHA * (p1 if n_pAp & 1 else p0), "the restatement")
        if n <= 4097 or special:
            assert run_x_finalize(gpu, block(x_pending=0, n_pAp=3, alpha=np.nan), x, p0, p1, what=(special, "not pending")) is x
        for alpha in (np.inf, -np.inf, np.nan, -0.0) if n <= 4097 else ():
            run_x_finalize(gpu, block(x_pending=1, alpha=alpha), x, p0, p1, what=(special, "alpha", alpha))


# ---- dot_spans_k<1|2>, waxpby_sdev_k ----------------------------------------------------------------------------------------------
def run_dot_spans(L, op, S, a, b, x, r, r_is_a=False, what=()):
    n = len(a)
    what = ("dot_spans_k", op, n) + tuple(what)
    want_x, want_r, want_q = ck.dot_spans(op, S, a, b, x, a if r_is_a else r)
    da, db = Buf(a), Buf(b)
    dx = Buf(x) if op == 1 else None
    dr = da if r_is_a else Buf(r) if op == 1 else Buf(n=n)
    dq = Buf(n=4 * ck.groups(n))
    d, i = S.d(), S.i()
    rc = L.sb_cg_dot_spans_native(op, n, da.ptr, db.ptr, ptr(dx), dr.ptr, dq.ptr, d.ctypes.data, i.ctypes.data)
    assert rc == 0, (what, "guard words around the control block changed", rc)
    same_block(ck.Block.from_arrays(d, i), S, what)
    if want_q is None:
        dq.kept(what + ("partials of a stopped launch",)), dr.kept(what + ("r of a stopped launch",))
        if dx:
            dx.kept(what + ("x of a stopped launch",))
    else:
        assert len(want_q) == 4 * ck.groups(n)
        dq.slots(want_q, what + ("level-0 partials",))
        assert not np.any(bits(dq.get(what)) == FILL_BITS), (what, "a partial below 4 ceil(n/256) was not written")
        same(dr.get(what + ("r",)), want_r, what + ("r",))
        if dx:
            same(dx.get(what + ("x",)), want_x, what + ("x",))
    if not r_is_a:
        da.kept(what + ("a",))
    db.kept(what + ("b",))
    free(da, db, dx, None if r_is_a else dr, dq)


@pytest.mark.parametrize("op", [1, 2])
@pytest.mark.parametrize("size", SMALL + BIG)
def test_dot_spans(gpu, sizes, size, op):
    """op 1: x += alpha p, r -= alpha Ap in place; op 2: r = b - Ap into its own vector and in place of b; the 4 ceil(n/256)
    level-0 partials of r.r; the stop flag"""
    n = sizes[size]
    for special in (False, True):
        r, p, x, Ap = vecs(n, special)
        run_dot_spans(gpu, op, block(), p, Ap, x, r, what=(special,))
        if op == 2:
            run_dot_spans(gpu, 2, block(alpha=np.nan), p, Ap, None, None, r_is_a=True, what=(special, "in place"))
    run_dot_spans(gpu, op, block(stop=1), p, Ap, x, r, what=("stopped",))
    if op == 1 and n <= 4097:
        for alpha in (np.inf, -np.inf, np.nan, -0.0):
            run_dot_spans(gpu, 1, block(alpha=alpha), p, Ap, x, r, what=("alpha", alpha))


def run_waxpby_sdev(L, S, x, y, negative, in_place, what=()):
    n = len(x)
    what = ("waxpby_sdev_k", n, "neg_alpha" if negative else "alpha", "in place" if in_place else "") + tuple(what)
    want = ck.waxpby_sdev(S, x, y, negative)
    dx, dy = Buf(x), Buf(y)
    dw = dx if in_place else Buf(n=n)
    d, i = S.d(), S.i()
    rc = L.sb_waxpby_sdev_native(n, dx.ptr, negative, dy.ptr, dw.ptr, d.ctypes.data, i.ctypes.data)
    assert rc == 0, (what, "guard words around the control block changed", rc)
    same_block(ck.Block.from_arrays(d, i), S, what)
    if want is None:
        dw.kept(what + ("w of a stopped launch",))
    else:
        same(dw.get(what + ("w",)), want, what + ("w",))
    if not in_place:
        dx.kept(what + ("x",))
    dy.kept(what + ("y",))
    free(dx, dy, None if in_place else dw)


@pytest.mark.parametrize("size", SMALL + BIG)
def test_waxpby_sdev(gpu, sizes, size):
    """w = x + (*scalar) y with the scalar at alpha / at neg_alpha, into its own vector and in place of x (as the loop's
    reference-shaped op list calls it); the stop flag"""
    n = sizes[size]
    for special in (False, True):
        r, p, x, Ap = vecs(n, special)
        S = block(neg_alpha=BETA)
        run_waxpby_sdev(gpu, S, x, p, 0, False, what=(special,))
        if n <= 4097 or not special:  # (past the grid's cap: once each)
            run_waxpby_sdev(gpu, S, x, p, 0, True, what=(special,))
            run_waxpby_sdev(gpu, S, r, Ap, 1, True, what=(special,))
    run_waxpby_sdev(gpu, block(stop=1), x, p, 1, True, what=("stopped",))
    if n <= 4097:
        run_waxpby_sdev(gpu, block(stop=1), x, p, 0, False, what=("stopped",))
    if n <= 4097:
        for alpha in (np.inf, -np.inf, np.nan, -0.0):
            run_waxpby_sdev(gpu, block(alpha=alpha), x, p, 0, True, what=("alpha", alpha))
