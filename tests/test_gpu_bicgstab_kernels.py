"""The kernels of BiCGStab alone, BIT FOR BIT against the CPU restatement's elementwise and tree-dot forms
(tests/bicgstab_ref.py): the p update, the s update, the dual dot (and the single dot the loop takes from dot_l1_k), the x / r
update with its two dots, and the scalar step's reduction -- at the sizes where the paths change (one lane, one span, the
partial last group, an odd n, more groups than waves, a second grid-stride trip of a capped grid), with NaN, +-Inf, -0.0 and
subnormals at distinct positions of distinct inputs, every output between sentinels."""
import numpy as np
import pytest

from oracle import pyoracle as po

import bicgstab_ref as ref
from sparsebench_amd.capi import DeviceVector

pytestmark = pytest.mark.gpu
SENTINEL = 9.9


def same(got, want, what):
    a, b = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), (what, "NaN positions differ", np.nonzero(na != nb)[0][:5])
    bad = np.nonzero((a.view(np.uint64) != b.view(np.uint64)) & ~na)[0]
    assert bad.size == 0, (what, "first difference at", int(bad[0]), a[bad[0]], b[bad[0]])


class Guarded:
    """n doubles on the device with two sentinel doubles in front and two behind (the payload stays 16-byte aligned)"""

    def __init__(self, data=None, n=None):
        self.n = len(data) if data is not None else n
        host = np.full(self.n + 4, SENTINEL)
        if data is not None:
            host[2:2 + self.n] = data
        self.dv = DeviceVector.from_host(host)
        self.ptr = self.dv.ptr + 16

    def get(self, what):
        a = self.dv.get()
        assert np.all(a[:2] == SENTINEL) and np.all(a[self.n + 2:] == SENTINEL), (what, "sentinel overwritten")
        return a[2:2 + self.n]

    def free(self):
        self.dv.free()


def specials(n, seed, count):
    """`count` random vectors with the special values at distinct positions of distinct vectors"""
    rng = np.random.default_rng(seed)
    v = [rng.standard_normal(n) for _ in range(count)]
    tiny = np.float64(5e-324)
    kinds = [np.nan, np.inf, -np.inf, -0.0, tiny, -tiny, 1e-310]
    for j, val in enumerate(kinds):
        for w in range(count):  # kind j of vector w
            for pos in {(19 * j + 3 * w + 1) % n, (n // 2 + 7 * j + w) % n, (n - 1 - 6 * j - w) % n}:
                v[w][pos] = val
    return v


def launch(L, n):
    out = np.zeros(3, dtype=np.uint32)
    L.sb_bicgstab_launch(n, out.ctypes.data)
    assert int(out[1]) == 1024
    return int(out[0]), int(out[2])


def sizes(L):
    """the paths of the streaming skeleton: one lane, one span, full and partial groups, an odd n, several groups per
    workgroup; 16 * 256 * grid(4097) + 257: one group more than the waves that grid has, then a partial odd one; and the grid
    is capped at 2 x CUs workgroups: the smallest n past the cap whose last, partial group is a wave's SECOND group"""
    grid, cus = launch(L, 4097)
    assert grid == 2
    out = [1, 63, 64, 255, 256, 257, 511, 513, 4097, 16 * 256 * grid + 257]
    cap, _ = launch(L, 0x7FFFFF00)
    assert cap == 2 * cus
    n = 256 * (cap * 16) + 257
    assert launch(L, n)[0] == cap
    return out + [n]


N_SIZES = 11


@pytest.fixture(scope="module")
def ns(gpu):
    s = sizes(gpu)
    assert len(s) == N_SIZES
    print("sizes:", s)
    return s


@pytest.mark.parametrize("i", range(N_SIZES))
def test_update_p(gpu, ns, i):
    n = ns[i]
    r, p, v, dinv = specials(n, 100 + i, 4)
    beta, omega = -0.37109375, 1.2890625
    want_p, want_ph = ref.update_p(r, p, v, dinv, beta, omega)
    dr, dp, dv, dd, dh = Guarded(r), Guarded(p), Guarded(v), Guarded(dinv), Guarded(n=n)
    gpu.sb_bicgstab_update_p_native(n, beta, omega, dr.ptr, dp.ptr, dv.ptr, dd.ptr, dh.ptr)
    same(dp.get("p"), want_p, (n, "p"))
    same(dh.get("ph"), want_ph, (n, "ph"))
    for d, a, w in ((dr, r, "r"), (dv, v, "v"), (dd, dinv, "dinv")):
        same(d.get(w), a, (n, w, "untouched"))
    for d in (dr, dp, dv, dd, dh):
        d.free()


def test_update_p_first_body_form(gpu):
    """beta = omega = 0.0 on zeroed p and v: p = r + 0.0 (so -0.0 becomes +0.0), whatever r holds"""
    n = 777
    r, dinv = specials(n, 7, 2)
    want_p, want_ph = ref.update_p(r, np.zeros(n), np.zeros(n), dinv, 0.0, 0.0)
    dr, dp, dv, dd, dh = Guarded(r), Guarded(np.zeros(n)), Guarded(np.zeros(n)), Guarded(dinv), Guarded(n=n)
    gpu.sb_bicgstab_update_p_native(n, 0.0, 0.0, dr.ptr, dp.ptr, dv.ptr, dd.ptr, dh.ptr)
    same(dp.get("p"), want_p, "p")
    same(dh.get("ph"), want_ph, "ph")
    for d in (dr, dp, dv, dd, dh):
        d.free()


@pytest.mark.parametrize("i", range(N_SIZES))
def test_update_s(gpu, ns, i):
    n = ns[i]
    r, v, dinv = specials(n, 200 + i, 3)
    alpha = 0.8203125
    want_s, want_sh = ref.update_s(r, v, dinv, alpha)
    inplace = i % 2 == 0  # the loop keeps s in r's storage
    dr, dv, dd, dh = Guarded(r), Guarded(v), Guarded(dinv), Guarded(n=n)
    ds = dr if inplace else Guarded(n=n)
    gpu.sb_bicgstab_update_s_native(n, alpha, dr.ptr, dv.ptr, dd.ptr, ds.ptr, dh.ptr)
    same(ds.get("s"), want_s, (n, "s"))
    same(dh.get("sh"), want_sh, (n, "sh"))
    if not inplace:
        same(dr.get("r"), r, (n, "r untouched"))
        ds.free()
    same(dv.get("v"), v, (n, "v untouched"))
    same(dd.get("dinv"), dinv, (n, "dinv untouched"))
    for d in (dr, dv, dd, dh):
        d.free()


@pytest.mark.parametrize("i", range(N_SIZES))
def test_dot2_pair_and_single(gpu, ns, i):
    n = ns[i]
    a, b = specials(n, 300 + i, 2)
    nG = (n + 255) // 256
    want_ab, tot_ab = ref.l1(a, b)
    want_aa, tot_aa = ref.l1(a, a)
    assert len(want_ab) == nG
    da, db = Guarded(a), Guarded(b)
    lab, laa = Guarded(n=nG), Guarded(n=nG)
    gpu.sb_bicgstab_dot2_native(n, 1, da.ptr, db.ptr, lab.ptr, laa.ptr)
    got_ab, got_aa = lab.get("l1 a.b"), laa.get("l1 a.a")
    same(got_ab, want_ab, (n, "pair a.b"))
    same(got_aa, want_aa, (n, "pair a.a"))
    same([po.reduce_final(got_ab), po.reduce_final(got_aa)], [tot_ab, tot_aa], (n, "totals"))
    one, untouched = Guarded(n=nG), Guarded(n=nG)
    gpu.sb_bicgstab_dot2_native(n, 0, da.ptr, db.ptr, one.ptr, untouched.ptr)
    same(one.get("l1 single"), want_ab, (n, "single a.b"))
    assert np.all(untouched.get("unused") == SENTINEL)
    same(da.get("a"), a, (n, "a untouched"))
    same(db.get("b"), b, (n, "b untouched"))
    for d in (da, db, lab, laa, one, untouched):
        d.free()


@pytest.mark.parametrize("i", range(N_SIZES))
def test_update_xr(gpu, ns, i):
    n = ns[i]
    x, ph, sh, s, t, rhat = specials(n, 400 + i, 6)
    alpha, omega = 0.8203125, -0.6484375
    want_x, want_r = ref.update_xr(x, ph, sh, s, t, alpha, omega)
    want_rho, tot_rho = ref.l1(rhat, want_r)
    want_rr, tot_rr = ref.l1(want_r, want_r)
    nG = (n + 255) // 256
    inplace = i % 2 == 1  # the loop keeps r in s's storage
    dx, dph, dsh, ds, dt, drh = (Guarded(a) for a in (x, ph, sh, s, t, rhat))
    dr = ds if inplace else Guarded(n=n)
    l_rho, l_rr = Guarded(n=nG), Guarded(n=nG)
    gpu.sb_bicgstab_update_xr_native(n, alpha, omega, dx.ptr, dph.ptr, dsh.ptr, ds.ptr, dt.ptr, drh.ptr, dr.ptr, l_rho.ptr, l_rr.ptr)
    same(dx.get("x"), want_x, (n, "x"))
    same(dr.get("r"), want_r, (n, "r"))
    got_rho, got_rr = l_rho.get("l1 rho"), l_rr.get("l1 rr")
    same(got_rho, want_rho, (n, "level-1 rhat.r"))
    same(got_rr, want_rr, (n, "level-1 r.r"))
    same([po.reduce_final(got_rho), po.reduce_final(got_rr)], [tot_rho, tot_rr], (n, "totals"))
    if not inplace:
        same(ds.get("s"), s, (n, "s untouched"))
        dr.free()
    for d, a, w in ((dph, ph, "ph"), (dsh, sh, "sh"), (dt, t, "t"), (drh, rhat, "rhat")):
        same(d.get(w), a, (n, w, "untouched"))
    for d in (dx, dph, dsh, ds, dt, drh, l_rho, l_rr):
        d.free()


@pytest.mark.parametrize("m", [1, 1023, 1025, 7168, 7169])
def test_scalar_reduction(gpu, m):
    """the scalar step's totals over m level-1 values: under, at and past one value per thread and the eight-deep unrolled trip
    of reduce_final_1024; on clean values of mixed magnitude (with -0.0 and subnormals), then with NaN and Inf planted"""
    rng = np.random.default_rng(m)
    a = rng.standard_normal(m) * np.exp2(rng.integers(-40, 40, m).astype(np.float64))
    b = rng.standard_normal(m) ** 2
    a[m // 3], b[m // 2], a[(2 * m) // 3] = -0.0, 5e-324, 1e-310
    for planted in (False, True):
        if planted:
            a[(5 * m) // 7], b[m - 1] = np.nan, np.inf
        da, db = Guarded(a), Guarded(b)
        out = np.full(2, SENTINEL)
        gpu.sb_bicgstab_reduce_native(m, da.ptr, db.ptr, out.ctypes.data)
        same(out, [po.reduce_final(a), po.reduce_final(b)], (m, planted))
        if not planted:
            assert np.isfinite(out).all()
        same(da.get("a"), a, "a untouched")
        da.free(), db.free()
