"""The single-precision CG loop's vector and scalar kernels alone: cg_update_p_f32<0|1>, cg_update_r_f32<0|1>,
cg_scalar_f32_k<0|1|2>, cg_local_f32_k, cg_apply_local_f32_k<0|1|2>, cg_x_finalize_f32, cg_x_finalize2_f32, axpy_sdev_f32_k,
dot_l1_f32_k and waxpby_f32_k with a stop flag, through the blocking entries that launch them with the loop's own launch
functions, each == its CPU restatement (tests/sp_cg_kernels_ref.py, pinned by tests/test_sp_cg_kernels_host.py) BIT FOR BIT as
uint32: NaN equal to NaN, -0.0 apart from +0.0, no tolerance.  The control block goes in and comes out as plain data and is
compared field by field.

Every device array sits between guards of quiet NaNs with a payload (64 floats in front, 512 behind its logical end; the data
pointer stays 16-byte aligned) that are compared as bits after the launch; what a launch may not write -- its inputs, and
everything on a set stop flag or a failed loop test -- is compared with its upload as bits; output slots (level-1 values,
histories) start as a payload NaN, so "exactly ceil(n/256) written" is literal.

Sizes: n = 1 .. 4 097 over all four n % 4 classes and a 256-group cut at each, and the sizes at which a thread / a wave of the
capped grid takes a second trip, derived from the launches the library reports (sb_cg_update_p_launch_f32,
sb_cg_update_r_launch_f32, sb_dot_l1_launch_f32, sb_stream_launch_f32) and printed, never written down here.  Every vector comes
in a finite variant (+0.0, -0.0, f32 subnormals at the first and last element, both sides of the 256-group boundary, n/2 and
n/3) and a special one (+-inf and a NaN there as well)."""
import numpy as np
import pytest

import sp_cg_kernels_ref as ck
import sp_ref
from sparsebench_amd.capi import DeviceVector

pytestmark = pytest.mark.gpu

F = np.float32
GUARD, FRONT = 512, 64
GUARD_BITS = 0x7FD00000  # + the word's index: quiet NaNs, every guard word another payload
FILL_BITS = np.uint32(0x7FCF1111)
SMALL = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097]
P_SIZES = ["p_stride-1", "p_stride", "p_stride+1", "p_2stride+1", "p_3stride+5"]
R_SIZES = ["r_one_trip", "r_one_group_more", "r_two_trips_257", "r_one_trip_1"]
D_SIZES = ["d_one_trip", "d_one_group_more", "d_two_trips_257", "d_one_trip_1"]
S_SIZES = ["s_cap+1", "s_2cap+3"]
ALPHA, BETA, NEG_ALPHA = 0.8046875, -1.2890625, -0.59375  # exactly representable, and neg_alpha is NOT -alpha
INEXACT = dict(alpha=0.1, beta=1.0 / 3.0, neg_alpha=-0.7)  # the double 1/3 is no float: the kernel narrows it
MAX_N = 7 << 20
SENTINEL = F(-7.5)


def fill(n):
    return np.full(n, FILL_BITS, dtype=np.uint32).view(F)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same(got, want, what):
    a, b = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), (what, "NaN positions differ", np.nonzero(na != nb)[0][:5])
    bad = np.nonzero((a.view(np.uint32) != b.view(np.uint32)) & ~na)[0]
    assert bad.size == 0, (what, "first difference at", int(bad[0]), a[bad[0]], b[bad[0]], "of", bad.size)


class Buf:
    """n floats on the device, 64 guard floats in front and 512 behind; data None: n payload-NaN slots"""

    def __init__(self, data=None, n=None):
        self.n = len(data) if data is not None else n
        up = np.uint32(GUARD_BITS) + (np.arange(FRONT + self.n + GUARD, dtype=np.uint32) & np.uint32(0xFFFFF))
        up[FRONT:FRONT + self.n] = bits(data) if data is not None else FILL_BITS
        self.up = up
        self.dv = DeviceVector.from_host(up.view(F), F)
        self.ptr = self.dv.ptr + 4 * FRONT
        assert self.ptr % 16 == 0

    def get(self, what):
        a = self.dv.get().view(np.uint32)
        lo, hi = FRONT, FRONT + self.n
        front, back = np.nonzero(a[:lo] != self.up[:lo])[0], np.nonzero(a[hi:] != self.up[hi:])[0]
        assert front.size == 0, (what, "guard in front overwritten at element", int(front[0]) - lo)
        assert back.size == 0, (what, "guard behind overwritten at element", self.n + int(back[0]))
        return a[lo:hi].copy().view(F)

    def kept(self, what):
        """payload and guards as uploaded, bit for bit"""
        got = bits(self.get(what))
        bad = np.nonzero(got != self.up[FRONT:FRONT + self.n])[0]
        assert bad.size == 0, (what, "changed at", int(bad[0]), "of", bad.size)

    def check(self, want, orig, what):
        """want is orig (the restatement's 'not written'): the upload's bits; else the restatement's values"""
        if want is orig or want is None:
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
    """r, p, x, Ap of n rows: slices of four vectors made once (mixed sign, magnitudes over 2^-12 .. 2^12), with the edge values
    at the first element, the last, both sides of the 256-group boundary, n/2 and n/3 -- another kind in each vector"""
    kinds = [0.0, -0.0, 1e-40, np.inf, -np.inf, np.nan] if special else [0.0, -0.0, 1e-40, -1e-40, 1e-45, -3e-39]
    out = []
    for w in range(4):
        if w not in _base:
            rng = np.random.default_rng(11 + w)
            _base[w] = rng.standard_normal(MAX_N, dtype=F) * np.exp2(rng.integers(-12, 13, MAX_N)).astype(F)
        v = _base[w][:n].copy()
        for j, pos in enumerate([0, n - 1, 255, 256, n // 2, n // 3]):
            if pos < n:
                v[pos] = kinds[(j + w) % 6]
        out.append(v)
    return out


def launch(L, what, n):
    out = np.zeros(3, dtype=np.uint32)
    getattr(L, "sb_%s_launch_f32" % what)(n, out.ctypes.data)
    return int(out[0]), int(out[1]), int(out[2])


@pytest.fixture(scope="module")
def sizes(gpu):
    """name -> n.  cg_update_p_f32: thread t of W x T takes the float4 t and t + W T; cg_update_r_f32 / dot_l1_f32_k: a wave per
    256-row group, 16 W waves; the 256-thread kernels: an element per thread of the capped grid"""
    s = {k: k for k in SMALL}
    W, T, cus = launch(gpu, "cg_update_p", 0x7FFFFF00)
    assert T == 1024 and W >= cus >= 1
    stride = W * T * 4
    for name, n in zip(P_SIZES, (stride - 1, stride, stride + 1, 2 * stride + 1, 3 * stride + 5)):
        s[name] = n
        assert launch(gpu, "cg_update_p", n)[0] == W, name
    assert launch(gpu, "cg_update_p", 1)[0] == 1 and launch(gpu, "cg_update_p", 4097)[0] == min(W, 2)
    print("cg_update_p_f32: %d workgroups x %d threads x 4 floats on %d CUs;" % (W, T, cus), {k: s[k] for k in P_SIZES})
    for what, names, kernel in (("cg_update_r", R_SIZES, "cg_update_r_f32"), ("dot_l1", D_SIZES, "dot_l1_f32_k")):
        W, T, _ = launch(gpu, what, 0x7FFFFF00)
        assert T == 1024 and W >= cus
        waves = W * (T // 64)
        for name, n in zip(names, (256 * waves, 256 * (waves + 1), 256 * 2 * waves + 257, 256 * waves + 1)):
            s[name] = n
            assert launch(gpu, what, n)[0] == W, name
        assert launch(gpu, what, 1)[0] == 1 and launch(gpu, what, 4097)[0] == min(W, 2)
        print("%s: %d workgroups, %d waves;" % (kernel, W, waves), {k: s[k] for k in names})
    W, T, _ = launch(gpu, "stream", 0x7FFFFF00)
    assert T == 256 and W >= cus
    for name, n in zip(S_SIZES, (W * T + 1, 2 * W * T + 3)):
        s[name] = n
        assert launch(gpu, "stream", n)[0] == W, name
    assert launch(gpu, "stream", 1)[0] == 1 and launch(gpu, "stream", 257)[0] == min(W, 2)
    print("the 256-thread kernels: %d workgroups x %d threads;" % (W, T), {k: s[k] for k in S_SIZES})
    assert max(s.values()) <= MAX_N
    return s


def same_block(got, want, what):
    same(got.f(), want.f(), what + ("control block", ck.FIELDS_F))
    gb, wb = got.b(), want.b()
    assert (np.isnan(gb[0]) and np.isnan(wb[0])) or gb.view(np.uint64)[0] == wb.view(np.uint64)[0], (what, "beta", gb, wb)
    assert np.array_equal(got.i(), want.i()), (what, "control block", [(f, int(a), int(b)) for f, a, b in zip(ck.FIELDS_I, got.i(), want.i()) if a != b])


def block(**kw):
    """a block of a running loop whose live rr / iters / stop_next differ from their snapshot twins"""
    base = dict(rr=3.5, rr_old=9.25, pAp=11.5, alpha=ALPHA, beta=BETA, neg_alpha=NEG_ALPHA, eps=1e-9, snap_rr=1.75, stop=0, stop_next=0,
                iters=7, n_rr=2, n_pAp=3, itermax=50, hist_cap=6, x_pending=0, snap_iters=4, snap_stop_next=0)
    base.update(kw)
    return ck.Block(**base)


class Blk:
    """the block as the three host arrays an entry takes and fills"""

    def __init__(self, S):
        self.f, self.b, self.i = S.f(), S.b(), S.i()
        self.args = (self.f.ctypes.data, self.b.ctypes.data, self.i.ctypes.data)

    def check(self, rc, want, what):
        assert rc == 0, (what, "guard words around the control block changed", rc)
        same_block(ck.Block.from_arrays(self.f, self.b, self.i), want, what)


def level1_values(m, seed, zero=False):
    """m positive level-1 values of mixed magnitude"""
    rng = np.random.RandomState(seed)
    return np.zeros(m, F) if zero else (rng.random_sample(m) * 10.0 ** rng.randint(-3, 4, size=m) + 2.0 ** -20).astype(F)


def big(size):
    return isinstance(size, str)


# ---- cg_update_p_f32 -----------------------------------------------------------------------------------------------------------
def run_update_p(L, mode, S, r, p, x, which, m=0, l1=None, hist=None, what=()):
    what = ("cg_update_p_f32", mode, len(r), "which", which) + tuple(what)
    want_S, want_p, want_x, want_h = ck.update_p(mode, S, r, p, x, which, m, l1, hist)
    dr, dp, dx = Buf(r), Buf(p), Buf(x) if x is not None else None
    dl, dh = Buf(l1) if l1 is not None else None, Buf(hist) if hist is not None else None
    B = Blk(S)
    rc = L.sb_cg_update_p_native_f32(mode, len(r), dr.ptr, dp.ptr, ptr(dx), which, m, ptr(dl), ptr(dh), *B.args)
    B.check(rc, want_S, what)
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


XCASES = ["no_x", "x_not_pending", "x_pending"]
P0_CASES = [(s, w, xc) for s in SMALL for w in (0, 1) for xc in XCASES] + [(s, 0, "x_pending") for s in P_SIZES] + [
    ("p_3stride+5", 1, "no_x"), ("p_3stride+5", 0, "x_not_pending"), ("p_2stride+1", 0, "no_x"), ("p_stride+1", 1, "x_pending")]


@pytest.mark.parametrize("size,which,xcase", P0_CASES)
def test_update_p_without_a_step(gpu, sizes, size, which, xcase):
    """cg_update_p_f32<0>: which = 1 is the literal r + 0.0 r (an infinite r gives NaN, -0.0 stays -0.0) and touches no x; the
    owed x update is taken on the OLD p, only with x and the pending flag; the block is not written"""
    n = sizes[size]
    for special in ((len(size) + which) & 1,) if big(size) else (0, 1):
        r, p, x, _ = vecs(n, special)
        S = block(x_pending=int(xcase == "x_pending"))
        xin = None if xcase == "no_x" else x
        _, wp, wx = run_update_p(gpu, 0, S, r, p, xin, which, what=(xcase, special))
        if which == 1:
            neg0 = bits(r) == bits(np.array([-0.0]))[0]
            assert np.all(bits(wp)[neg0] == bits(np.array([-0.0]))[0]) and np.all(np.isnan(wp[np.isinf(r)]))
        assert (wx is not xin) == (xcase == "x_pending" and which == 0)


@pytest.mark.parametrize("size", [5, 1025])
def test_update_p_inexact_coefficients(gpu, sizes, size):
    """alpha = float(0.1), beta = the DOUBLE 1/3 narrowed by the kernel: every product is rounded before its add"""
    r, p, x, _ = vecs(sizes[size], 0)
    S = block(x_pending=1, **INEXACT)
    _, wp, wx = run_update_p(gpu, 0, S, r, p, x, 0, what=("inexact",))
    with np.errstate(all="ignore"):
        same(wp, r + F(np.float64(1.0) / 3.0) * p, "p"), same(wx, x + F(0.1) * p, "x")


@pytest.mark.parametrize("size", [3, 257, 4097, "p_stride+1"])
def test_update_p_stopped_changes_nothing(gpu, sizes, size):
    n = sizes[size]
    r, p, x, _ = vecs(n, 1)
    for mode, which in ((0, 0), (0, 1), (1, 0)):
        l1, hist = (level1_values(5, 1), fill(6)) if mode else (None, None)
        wS, wp, wx = run_update_p(gpu, mode, block(stop=1, x_pending=1), r, p, x, which, 5 if mode else 0, l1, hist, what=("stopped",))
        assert wp is p and wx is x


@pytest.mark.parametrize("size", SMALL + P_SIZES)
def test_update_p_with_the_beta_step(gpu, sizes, size):
    """cg_update_p_f32<1> at every size: the loop test passes, the vectors' beta = F(total / snap_rr) while the block keeps the
    recorder's double of F(total / rr); the x update is owed with x given, whatever x_pending says"""
    n = sizes[size]
    m = 37
    l1 = level1_values(m, n % 97)
    for special in ((len(size) & 1),) if big(size) else (0, 1):
        r, p, x, _ = vecs(n, special)
        S = block()
        wS, wp, wx = run_update_p(gpu, 1, S, r, p, x if not special else None, 0, m, l1, fill(6), what=(special,))
        total = ck.total_of(l1, m, 1)
        assert wS.beta == np.float64(F(total / S.rr)) != np.float64(F(total / S.snap_rr)) and wS.rr == total and wS.rr_old == S.rr
        with np.errstate(all="ignore"):
            same(wp, r + F(total / S.snap_rr) * p, "p from snap_rr")
        assert special or wx is not x


FOLD_P = {
    "passes": {},
    "fails_on_itermax": dict(itermax=5),                                     # snap_iters + 1 == itermax (the live test fails too)
    "fails_on_itermax_in_the_snapshot_only": dict(itermax=9, snap_iters=8),  # live: 7 + 1 < 9
    "passes_in_the_snapshot_only": dict(itermax=6),                          # live: 7 + 1 < 6 fails, the snapshot's 4 + 1 < 6 passes
    "fails_on_snap_stop_next": dict(snap_stop_next=1, stop_next=1),
    "fails_on_snap_stop_next_in_the_snapshot_only": dict(snap_stop_next=1),
    "stop_next_live_only": dict(stop_next=1),
    "stopped": dict(stop=1),
    "history_full": dict(n_rr=6),
    "history_one_left": dict(n_rr=5),
    "history_of_no_entries": dict(n_rr=0, hist_cap=0),
    "x_pending_already": dict(x_pending=1),
    "converges": dict(eps=1e30),
    "snap_rr_zero": dict(snap_rr=0.0),
    "total_nan": {},
    "inexact": dict(INEXACT),
}


@pytest.mark.parametrize("scenario", list(FOLD_P))
def test_update_p_beta_step_scenarios(gpu, sizes, scenario):
    """the loop test from the SNAPSHOT (snap_iters, snap_stop_next), beta from snap_rr -- the live rr / iters / stop_next differ
    from them, as they do for a late workgroup once the recorder has stored the step; the recorded step from the block as it
    was.  A set stop flag writes nothing, a failed test the block alone; at n_rr == hist_cap no history store, n_rr advances.
    (Where the live test fails and the snapshot's passes -- which no loop produces: the alpha step copies one from the other --
    the recorder raises `stop` while the vectors move, and a workgroup that starts late would see it: one workgroup only.)"""
    m = 5
    l1 = level1_values(m, 3)
    if scenario == "total_nan":
        l1[2] = np.nan
    one_workgroup = scenario in ("passes_in_the_snapshot_only", "stop_next_live_only")
    for n in (5, 1025) if one_workgroup else (5, 1025, sizes["p_stride+1"]):
        r, p, x, _ = vecs(n, 0)
        S = block(**FOLD_P[scenario])
        wS, wp, wx = run_update_p(gpu, 1, S, r, p, x, 0, m, l1, fill(S.hist_cap), what=(scenario,))
        if scenario in ("passes", "history_full", "history_one_left", "passes_in_the_snapshot_only", "stop_next_live_only"):
            assert wp is not p and wx is not x
        if scenario.startswith("fails"):
            assert wp is p and wx is x and wS.x_pending == 1
        if scenario == "history_full":
            assert wS.n_rr == 7
        if scenario == "history_one_left":
            assert wS.n_rr == 6
        if scenario == "stopped":
            assert wS is S and wp is p and wx is x
        if scenario in ("passes_in_the_snapshot_only", "stop_next_live_only"):
            assert wS.stop == 1  # (the recorder's live test failed while the vectors moved)


@pytest.mark.parametrize("m", [1, 16, 1023, 1024, 1025, 2049])
def test_update_p_total_of_m_level1_values(gpu, m):
    """cg_update_p_f32<1>: every workgroup reduces the m level-1 values itself; a thread of the 1024 takes 1, 2 and 3 of them"""
    for n in (257, 4097):
        r, p, x, _ = vecs(n, 0)
        wS, wp, _ = run_update_p(gpu, 1, block(), r, p, x, 0, m, level1_values(m, m), fill(6), what=("m", m))
        assert wS.rr == ck.total_of(level1_values(m, m), m, 1) and wp is not p


def test_update_p_beta_step_of_no_rows(gpu):
    """n = 0, m = 0: the loop launches the kernel for its step alone; the total of no values is +0.0"""
    e = np.zeros(0, F)
    for kw in ({}, dict(stop=1), dict(itermax=5)):
        S = block(**kw)
        wS, wp, wx = run_update_p(gpu, 1, S, e, e, e, 0, 0, e, fill(6), what=("no rows",))
        assert wp is e and wx is e and (wS is S) == bool(kw.get("stop"))
        if not kw:
            assert bits(wS.rr)[0] == 0 and wS.n_rr == 3 and wS.x_pending == 1


@pytest.mark.parametrize("coeff", [np.inf, -np.inf, np.nan, 0.0, -0.0])
def test_update_p_special_coefficients(gpu, coeff):
    for n in (257, 1023):
        for special in (0, 1):
            r, p, x, _ = vecs(n, special)
            run_update_p(gpu, 0, block(beta=coeff, x_pending=1), r, p, x, 0, what=("beta", coeff))
            run_update_p(gpu, 0, block(alpha=coeff, x_pending=1), r, p, x, 0, what=("alpha", coeff))
            run_update_p(gpu, 1, block(alpha=coeff, snap_rr=coeff), r, p, x, 0, 3, level1_values(3, 2), fill(6), what=("alpha and snap_rr", coeff))


# ---- cg_update_r_f32 -----------------------------------------------------------------------------------------------------------
def run_update_r(L, mode, S, Ap, r, m=0, l1in=None, rr_hist=None, pAp_hist=None, what=()):
    n = len(r)
    what = ("cg_update_r_f32", mode, n) + tuple(what)
    want_S, want_r, want_l1, want_rh, want_ph = ck.update_r(mode, S, Ap, r, m, l1in, rr_hist, pAp_hist)
    dA, dr, do = Buf(Ap), Buf(r), Buf(n=ck.groups(n))
    dl = Buf(l1in) if l1in is not None else None
    drh, dph = Buf(rr_hist) if rr_hist is not None else None, Buf(pAp_hist) if pAp_hist is not None else None
    B = Blk(S)
    rc = L.sb_cg_update_r_native_f32(mode, n, dA.ptr, dr.ptr, do.ptr, m, ptr(dl), ptr(drh), ptr(dph), *B.args)
    B.check(rc, want_S, what)
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
        drh.kept(what + ("rr history: never written by this kernel",))
    if dph:
        dph.slots(want_ph, what + ("pAp history",))
    free(dA, dr, do, dl, drh, dph)
    return want_S, want_r, want_l1


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("size", SMALL + R_SIZES)
def test_update_r(gpu, sizes, size, mode):
    """r += nalpha Ap and the level-1 values of r.r: exactly ceil(n/256) slots.  mode 0 reads neg_alpha (which is not -alpha
    here); mode 1 forms -(rr / total) and records cg_apply_f32<2>: alpha, neg_alpha, pAp, the pAp history, n_pAp, x_pending
    cleared, the snapshot copies"""
    n = sizes[size]
    m = 41
    for special in ((len(size) + mode) & 1,) if big(size) else (0, 1):
        r, _, _, Ap = vecs(n, special)
        if mode == 0:
            _, wr, _ = run_update_r(gpu, 0, block(), Ap, r, what=(special,))
            with np.errstate(all="ignore"):
                same(wr, r + F(NEG_ALPHA) * Ap, "r")
        else:
            l1 = level1_values(m, n % 89)
            wS, _, _ = run_update_r(gpu, 1, block(x_pending=1), Ap, r, m, l1, fill(6), fill(6), what=(special,))
            assert (wS.snap_rr, wS.snap_iters, wS.snap_stop_next, wS.x_pending, wS.n_pAp) == (F(3.5), 7, 0, 0, 4)
            assert wS.alpha == F(F(3.5) / ck.total_of(l1, m, 1)) and wS.neg_alpha == -wS.alpha


FOLD_R = {
    "passes": {},
    "stopped": dict(stop=1),
    "history_full": dict(n_pAp=6),
    "history_one_left": dict(n_pAp=5),
    "history_of_no_entries": dict(n_pAp=0, hist_cap=0),
    "stop_next_is_copied": dict(stop_next=1),
    "x_pending_is_cleared": dict(x_pending=1),
    "total_zero": {},                      # alpha = rr / 0 = +inf
    "total_zero_rr_zero": dict(rr=0.0),    # alpha = NaN
    "total_zero_rr_negative": dict(rr=-3.5),
    "total_nan": {},
    "inexact": dict(INEXACT, rr=0.7),
}


@pytest.mark.parametrize("scenario", list(FOLD_R))
@pytest.mark.parametrize("mode", [0, 1])
def test_update_r_alpha_step_scenarios(gpu, sizes, mode, scenario):
    kw = dict(FOLD_R[scenario])
    m = 5
    l1 = level1_values(m, 4, zero=scenario.startswith("total_zero"))
    if scenario == "total_nan":
        l1[4] = np.nan
    if mode == 0:  # the coefficient is the block's neg_alpha: the one the scenario's total would have given
        kw["neg_alpha"] = {"total_zero": -np.inf, "total_zero_rr_zero": np.nan, "total_zero_rr_negative": np.inf,
                           "total_nan": np.nan}.get(scenario, kw.get("neg_alpha", NEG_ALPHA))
    for n in (5, 1025, sizes["r_one_group_more"]):
        for special in (0, 1) if n < 4096 else (0,):
            r, _, _, Ap = vecs(n, special)
            S = block(**kw)
            hists = (fill(S.hist_cap), fill(S.hist_cap)) if mode else (None, None)
            wS, wr, wl = run_update_r(gpu, mode, S, Ap, r, m if mode else 0, l1 if mode else None, *hists, what=(scenario, special))
            if scenario == "stopped":
                assert wS is S and wr is r and wl is None
            elif mode and scenario == "history_full":
                assert wS.n_pAp == 7
            elif mode and scenario == "x_pending_is_cleared":
                assert wS.x_pending == 0
            elif mode and scenario == "stop_next_is_copied":
                assert wS.snap_stop_next == 1
            elif mode and scenario == "total_zero":
                assert wS.alpha == np.inf and wS.neg_alpha == -np.inf and not np.isfinite(wr[Ap != 0]).any()
            elif mode and scenario == "total_zero_rr_zero":
                assert np.isnan(wS.alpha) and np.isnan(wr).all()


@pytest.mark.parametrize("m", [1, 16, 1023, 1024, 1025, 2049])
def test_update_r_total_of_m_level1_values(gpu, m):
    for n in (257, 4097):
        r, _, _, Ap = vecs(n, 0)
        wS, _, _ = run_update_r(gpu, 1, block(), Ap, r, m, level1_values(m, m + 1), fill(6), fill(6), what=("m", m))
        assert wS.pAp == ck.total_of(level1_values(m, m + 1), m, 1)


# ---- cg_scalar_f32_k, cg_local_f32_k, cg_apply_local_f32_k ------------------------------------------------------------------------
def run_scalar(L, mode, split, S, q, m, defer_x, l1, what=()):
    """split 0: the step in one launch; 1: the sum alone into `local`; 2: the step alone on the sum the restatement gives"""
    what = ("scalar step", mode, "split", split, "m", m, "defer_x", defer_x, "l1", l1) + tuple(what)
    rh, ph = fill(S.hist_cap), fill(S.hist_cap)
    total = ck.total_of(q, m, l1)
    if split == 0:
        want_S, want_rh, want_ph = ck.scalar(mode, S, q, m, defer_x, l1, rh, ph)
        loc_in = loc_want = SENTINEL
    elif split == 1:
        want_S, want_rh, want_ph = S, rh, ph
        loc_in = SENTINEL
        loc_want = ck.local(S, q, m, l1, SENTINEL)
    else:
        want_S, want_rh, want_ph = ck.apply_local(mode, S, total, defer_x, rh, ph)
        loc_in = loc_want = total
    dq, drh, dph = Buf(q), Buf(rh), Buf(ph)
    B = Blk(S)
    loc = np.array([loc_in], dtype=F)
    rc = L.sb_cg_scalar_native_f32(mode, split, m, dq.ptr, drh.ptr, dph.ptr, defer_x, l1, *B.args, loc.ctypes.data)
    B.check(rc, want_S, what)
    same(loc, np.array([loc_want], F), what + ("local",))
    dq.kept(what + ("q",))
    drh.slots(want_rh, what + ("rr history",))
    dph.slots(want_ph, what + ("pAp history",))
    free(dq, drh, dph)
    return want_S


ROOT2 = F(np.sqrt(np.float64(F(2.0))))  # the float the double root of 2 is stored to
SCALAR = {
    "runs": (5.25, {}),
    "stopped": (5.25, dict(stop=1)),
    "history_full": (5.25, dict(n_rr=6, n_pAp=6)),
    "history_one_left": (5.25, dict(n_rr=5, n_pAp=5)),
    "history_of_no_entries": (5.25, dict(n_rr=0, n_pAp=0, hist_cap=0)),
    "itermax_1": (5.25, dict(itermax=1, iters=0)),
    "itermax_2": (5.25, dict(itermax=2, iters=0)),
    "last_body": (5.25, dict(itermax=9)),
    "stop_next_set": (5.25, dict(stop_next=1)),
    "total_zero": (0.0, {}),
    "total_nan": (np.nan, {}),
    "total_negative": (-2.0, {}),
    "total_inexact": (0.3, dict(rr=0.7)),
    "norm_equals_eps": (F(2.0), dict(eps=ROOT2)),
    "norm_one_float_above": (np.nextafter(F(2.0), F(4.0)), dict(eps=ROOT2)),
}


def test_the_two_totals_straddle_eps():
    """picked on the CPU: F(sqrt(float64(2))) is eps exactly, which fails `normr > eps`; the next float above 2 passes"""
    lo, hi = SCALAR["norm_equals_eps"][0], SCALAR["norm_one_float_above"][0]
    assert bits(hi)[0] == bits(lo)[0] + 1
    assert F(np.sqrt(np.float64(lo))) == ROOT2 and sp_ref.normr_fails(lo, ROOT2) and not sp_ref.normr_fails(hi, ROOT2)


@pytest.mark.parametrize("scenario", list(SCALAR))
@pytest.mark.parametrize("split", [0, 1, 2])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_scalar_step(gpu, mode, split, scenario):
    """every mode x split x l1 x defer_x on one value: as one level-1 value (m = 1, l1 = 1: the seq dot's shape) and as four
    level-0 partials; sqrt(total) > eps decided by one float; NaN and negative totals fail it"""
    total, kw = SCALAR[scenario]
    S = block(**kw)
    with np.errstate(all="ignore"):
        for l1 in (1, 0):
            q = np.array([total, 0.0] if l1 else [total, 0.0, 0.0, 0.0], F)
            for defer_x in (0, 1):
                wS = run_scalar(gpu, mode, split, S, q, 1, defer_x, l1, what=(scenario,))
                if split == 1 or scenario == "stopped":
                    assert wS is S
                    continue
                if scenario.startswith("norm") and mode < 2:
                    assert wS.stop_next == int(scenario == "norm_equals_eps")
                if scenario in ("total_nan", "total_negative", "total_zero") and mode == 0:
                    assert wS.stop_next == 1 and wS.stop == 1
                if scenario == "itermax_1" and mode == 0:
                    assert wS.stop == 1 and wS.iters == 0
                if scenario == "itermax_2" and mode == 0:
                    assert wS.stop == 0 and wS.iters == 1
                if mode == 1:
                    assert wS.x_pending == defer_x


@pytest.mark.parametrize("m", [1, 3, 1023, 1024, 1025, 2049])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_scalar_step_reduces_m_values(gpu, mode, m):
    for l1 in (1, 0):
        q = level1_values(m if l1 else 4 * m, 7 * m + l1)
        for split in (0, 1, 2):
            wS = run_scalar(gpu, mode, split, block(), q, m, 1, l1, what=("reduction",))
            if split != 1:
                assert (wS.pAp if mode == 2 else wS.rr) == ck.total_of(q, m, l1)


# ---- cg_x_finalize_f32, cg_x_finalize2_f32 --------------------------------------------------------------------------------------
def run_x_finalize(L, S, x, p0, p1, what=()):
    what = ("cg_x_finalize%s_f32" % ("2" if p1 is not None else ""), len(x)) + tuple(what)
    want = ck.x_finalize(S, x, p0, p1)
    dx, d0, d1 = Buf(x), Buf(p0), Buf(p1) if p1 is not None else None
    B = Blk(S)
    rc = L.sb_cg_x_finalize_native_f32(len(x), dx.ptr, d0.ptr, ptr(d1), *B.args)
    B.check(rc, S, what)
    dx.check(want, x, what + ("x",))
    d0.kept(what + ("p0",))
    if d1:
        d1.kept(what + ("p1",))
    free(dx, d0, d1)
    return want


@pytest.mark.parametrize("size", SMALL + S_SIZES)
def test_x_finalize(gpu, sizes, size):
    """x += alpha p only where the update is pending; one buffer, or the one of two that n_pAp names (odd: p1) -- they differ"""
    n = sizes[size]
    for special in (len(size) & 1,) if big(size) else (0, 1):
        _, p0, x, p1 = vecs(n, special)
        for n_pAp in (4, 7):
            want = run_x_finalize(gpu, block(x_pending=1, n_pAp=n_pAp), x, p0, p1, what=(special, n_pAp))
            with np.errstate(all="ignore"):
                same(want, x + F(ALPHA) * (p1 if n_pAp & 1 else p0), "the restatement")
        want = run_x_finalize(gpu, block(x_pending=1, n_pAp=7), x, p0, None, what=(special, "one buffer"))
        with np.errstate(all="ignore"):
            same(want, x + F(ALPHA) * p0, "the restatement")
        assert run_x_finalize(gpu, block(x_pending=0, n_pAp=3, alpha=np.nan), x, p0, p1, what=(special, "not pending")) is x
        assert run_x_finalize(gpu, block(x_pending=0, alpha=np.nan), x, p0, None, what=(special, "not pending")) is x
        for alpha in (np.inf, -np.inf, np.nan, -0.0, 0.1) if not big(size) else ():
            run_x_finalize(gpu, block(x_pending=1, alpha=alpha), x, p0, p1, what=(special, "alpha", alpha))
            run_x_finalize(gpu, block(x_pending=1, alpha=alpha), x, p0, None, what=(special, "alpha", alpha))


# ---- axpy_sdev_f32_k, dot_l1_f32_k, waxpby_f32_k with a stop flag ----------------------------------------------------------------
def run_axpy_sdev(L, S, x, y, negative, in_place, what=()):
    n = len(x)
    what = ("axpy_sdev_f32_k", n, "neg_alpha" if negative else "alpha", "in place" if in_place else "") + tuple(what)
    want = ck.axpy_sdev(S, x, y, negative)
    dx, dy = Buf(x), Buf(y)
    dw = dx if in_place else Buf(n=n)
    B = Blk(S)
    rc = L.sb_axpy_sdev_native_f32(n, dx.ptr, negative, dy.ptr, dw.ptr, *B.args)
    B.check(rc, S, what)
    dw.check(want, None, what + ("w",))
    if not in_place:
        dx.kept(what + ("x",))
    dy.kept(what + ("y",))
    free(dx, dy, None if in_place else dw)
    return want


@pytest.mark.parametrize("size", SMALL + S_SIZES)
def test_axpy_sdev(gpu, sizes, size):
    """w = x + (*scalar) y with the scalar at alpha / at neg_alpha, in place of x (the loop's use) and into its own vector; the
    stop flag"""
    n = sizes[size]
    for special in (len(size) & 1,) if big(size) else (0, 1):
        r, p, x, Ap = vecs(n, special)
        S = block()
        with np.errstate(all="ignore"):
            same(run_axpy_sdev(gpu, S, x, p, 0, True, what=(special,)), x + F(ALPHA) * p, "x")
            same(run_axpy_sdev(gpu, S, r, Ap, 1, True, what=(special,)), r + F(NEG_ALPHA) * Ap, "r")
        if not big(size):
            run_axpy_sdev(gpu, S, x, p, 0, False, what=(special,))
            run_axpy_sdev(gpu, block(**INEXACT), x, p, 1, True, what=(special, "inexact"))
    assert run_axpy_sdev(gpu, block(stop=1), x, p, 1, True, what=("stopped",)) is None
    if not big(size):
        assert run_axpy_sdev(gpu, block(stop=1), x, p, 0, False, what=("stopped",)) is None
        for alpha in (np.inf, -np.inf, np.nan, -0.0):
            run_axpy_sdev(gpu, block(alpha=alpha), x, p, 0, True, what=("alpha", alpha))


def run_dot_l1(L, a, b, stopped, what=()):
    n = len(a)
    what = ("dot_l1_f32_k", n, "stopped" if stopped else "") + tuple(what)
    want = ck.dot_l1(a, b, stopped)
    da, db = Buf(a), Buf(b) if b is not a else None
    do = Buf(n=ck.groups(n))
    rc = L.sb_dot_l1_native_f32(n, da.ptr, (db or da).ptr, do.ptr, stopped)
    assert rc == 0, (what, "guard words around the stop flag changed", rc)
    if want is None:
        do.kept(what + ("level-1 values of a stopped launch",))
    else:
        assert len(want) == ck.groups(n)
        do.slots(want, what + ("level-1 values",))
        assert not np.any(bits(do.get(what)) == FILL_BITS), (what, "a level-1 slot below ceil(n/256) was not written")
    da.kept(what + ("a",))
    if db:
        db.kept(what + ("b",))
    free(da, db, do)


@pytest.mark.parametrize("size", SMALL + D_SIZES)
def test_dot_l1(gpu, sizes, size):
    """the ceil(n/256) level-1 values of p . Ap and of r . r (one vector twice); nothing on a set flag"""
    n = sizes[size]
    for special in (len(size) & 1,) if big(size) else (0, 1):
        r, p, _, Ap = vecs(n, special)
        run_dot_l1(gpu, p, Ap, 0, what=(special,))
        if not big(size):
            run_dot_l1(gpu, r, r, 0, what=(special, "r.r"))
    if not big(size) or size == "d_one_group_more":
        run_dot_l1(gpu, p, Ap, 1)


BRANCHES = [(1.0, 0.37), (-0.71, 1.0), (2.5, -1.25), (1.0, 1.0), (1.0, 0.0)]  # alpha == 1 | beta == 1 | neither | both | r + 0.0 r


def run_waxpby_stop(L, alpha, x, beta, y, stopped, alias, what=()):
    n = len(x)
    what = ("waxpby_f32_k", n, alpha, beta, "stopped" if stopped else "", alias) + tuple(what)
    want = ck.waxpby_stop(alpha, x, beta, y, stopped)
    dx, dy = Buf(x), Buf(y)
    dw = dx if alias == "x" else dy if alias == "y" else Buf(n=n)
    rc = L.sb_waxpby_stop_native_f32(n, alpha, dx.ptr, beta, dy.ptr, dw.ptr, stopped)
    assert rc == 0, (what, "guard words around the stop flag changed", rc)
    dw.check(want, None, what + ("w",))
    if alias != "x":
        dx.kept(what + ("x",))
    if alias != "y":
        dy.kept(what + ("y",))
    free(dx, dy, dw if alias == "none" else None)


@pytest.mark.parametrize("size", SMALL + S_SIZES)
def test_waxpby_with_a_stop_flag(gpu, sizes, size):
    """the three branches (and alpha == beta == 1, and the loop's r + 0.0 r) with a clear flag and a set one; w its own vector,
    x (src/CGSolver.c:127) and y (:114)"""
    n = sizes[size]
    for k, (alpha, beta) in enumerate(BRANCHES[:3] if big(size) else BRANCHES):
        for special in ((k + len(size)) & 1,) if big(size) else (0, 1):
            r, p, x, _ = vecs(n, special)
            run_waxpby_stop(gpu, alpha, x, beta, p, 0, ("none", "x", "y")[k % 3], what=(special,))
            if not big(size):
                run_waxpby_stop(gpu, alpha, r, beta, p, 0, ("y", "none", "x")[k % 3], what=(special,))
                run_waxpby_stop(gpu, alpha, x, beta, p, 1, "x", what=(special,))
    run_waxpby_stop(gpu, 2.5, x, -1.25, p, 1, "none")
