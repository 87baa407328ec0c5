"""The kernels of the Chebyshev-smoothed V-cycle alone, BIT FOR BIT against the CPU restatement (tests/precond_ref.py,
pinned by tests/test_mg_poly_host.py), NaN equal to NaN: mgp_first_k through its native entry at the sizes where its paths change
-- fewer rows than one wave's span, the partial last group, an odd n, every wave on a second trip of its group loop -- with +0.0,
-0.0, denormals, an inf and a NaN in every vector, a stale inf and NaN in d, and guard doubles behind them; mgp_restrict_k and the
prolongation through sb_pcg_mg_poly_probe on mg_cases' shapes in every format and on a caller's hierarchy with an empty row of P
and a stored weight of 0.0; every level's interval and coefficients; and one whole cycle through sb_pcg_apply_precond at steps
1 .. 3 in both kernel modes of the SpMV."""
import numpy as np
import pytest

from oracle import pyoracle as po

import mg_poly_cases as cases
import pcg_ref
import precond_ref as ref
from sparsebench_amd import hostapi
from sparsebench_amd.capi import DeviceVector
from test_gpu_poly_kernels import same, vectors, guarded, check_guarded, modes, GUARD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("mg_poly_kernels")


def two_trips_n(L):
    """the smallest n with a partial, odd last group at which EVERY wave of the launch makes at least two trips of its group
    loop: twice as many full groups as the grid at its cap has waves, then 257 rows -- from the launch the library reports"""
    out = np.zeros(3, dtype=np.uint32)
    L.sb_pcg_mg_poly_first_launch(0x7FFFFF00, out.ctypes.data)
    cap, threads, cus = int(out[0]), int(out[1]), int(out[2])
    assert threads == 1024 and cap >= cus >= 1
    n = 256 * 2 * cap * (threads // 64) + 257
    L.sb_pcg_mg_poly_first_launch(n, out.ctypes.data)
    assert int(out[0]) == cap
    return n


def first_ref(r, w, dinv, z, c1):
    """mgp_first_k: (d, z, the level-1 values of r.z)"""
    with np.errstate(all="ignore"):
        u = r - w
        u = u * dinv
        d = u * np.float64(c1)
        zn = z + d
        return d, zn, po.ddot_partials(np.ascontiguousarray(r), zn)


@pytest.mark.parametrize("n", cases.KERNEL_N + ["two_trips"])
def test_first_native_equals_the_restatement(gpu, n):
    L = gpu
    if n == "two_trips":
        n = two_trips_n(L)
        print("every wave makes two trips at n =", n)
    r, w, dinv, z, stale = vectors(n, seed=(n + 11) % 1000, count=5)
    c1 = 0.94140625
    nG = (n + 255) // 256
    want_d, want_z, want_l1 = first_ref(r, w, dinv, z, c1)
    assert len(want_l1) == nG
    if n > 5:
        assert np.isnan(want_z).any() and np.isnan(stale).any() and np.isinf(stale).any()  # the special values reach the result
    for last in (0, 1):
        what = (n, "last", last)
        dr, dw, di, dd, dz = guarded(r), guarded(w), guarded(dinv), guarded(stale), guarded(z)  # d holds a stale inf and NaN
        dl = DeviceVector.from_host(np.full(nG + 4, GUARD))
        L.sb_pcg_mg_poly_first_native(n, last, c1, dr.ptr, dw.ptr, di.ptr, dd.ptr, dz.ptr, dl.ptr)
        check_guarded(dd, want_d, what + ("d",))
        check_guarded(dz, want_z, what + ("z",))
        check_guarded(dr, r, what + ("r untouched",))
        check_guarded(dw, w, what + ("w untouched",))
        check_guarded(di, dinv, what + ("dinv untouched",))
        check_guarded(dl, want_l1 if last else np.zeros(0), what + ("level-1 r.z",))
        for v in (dr, dw, di, dd, dz, dl):
            v.free()


def test_first_keeps_the_sign_of_a_zero_and_gives_the_tree_dot(gpu):
    """z = -0.0 with d = -0.0 stays -0.0 (poly_step_k with a = 0 would add +0.0 and lose it); on clean data the level-1 values
    sum to the tree dot"""
    n = 5000
    rng = np.random.default_rng(5)
    r, w, dinv, z = rng.standard_normal(n), rng.standard_normal(n), 1.0 + rng.random(n), rng.standard_normal(n)
    r[7], w[7], z[7] = -1.0, -1.0, -0.0  # u = -1 - -1 = +0.0 ... d = +0.0, z = -0.0 + +0.0 = +0.0
    r[9], w[9], z[9], dinv[9] = 0.0, 5e-324, -0.0, 1.0  # u = -5e-324, d = u * c1 rounds to -0.0 for c1 = 0.25, z = -0.0
    want_d, want_z, want_l1 = first_ref(r, w, dinv, z, 0.25)
    assert want_d[9] == 0.0 and np.signbit(want_d[9]) and np.signbit(want_z[9]) and not np.signbit(want_z[7])
    assert po.reduce_final(want_l1) == po.ddot_tree(r, want_z)
    dr, dw, di, dd, dz = (DeviceVector.from_host(v) for v in (r, w, dinv, np.full(n, np.nan), z))
    dl = DeviceVector((n + 255) // 256)
    gpu.sb_pcg_mg_poly_first_native(n, 1, 0.25, dr.ptr, dw.ptr, di.ptr, dd.ptr, dz.ptr, dl.ptr)
    same(dd.get(), want_d, "d"), same(dz.get(), want_z, "z"), same(dl.get(), want_l1, "level-1 r.z")
    for v in (dr, dw, di, dd, dz, dl):
        v.free()


def fused_dot(p, fmt, C):
    return (fmt == "scs" and C == 64) or p.use_packed(5) == 5


def check_handle(s, p, hier, fmt, C, what, cycles=True):
    """levels, rows, steps, intervals, coefficients, launches, bytes, every level's transfers on their own and whole cycles"""
    op = hier.lev[0].op
    assert s.precond() == "mgpoly" and s.levels() == hier.L and s.colours() == 0, (what, s.precond(), s.levels(), hier.L)
    assert [s.level_rows(l) for l in range(hier.L)] == [V.n for V in hier.lev], what
    assert [s.level_colours(l) for l in range(hier.L)] == [0] * hier.L and s.steps() == hier.steps
    for l, V in enumerate(hier.lev):
        assert s.level_steps(l) == V.smoother.steps == (hier.coarse_steps if l == hier.L - 1 else hier.steps)
        assert s.interval(l) == (V.smoother.c["lmin"], V.smoother.c["lmax"]), (what, l)
        same(s.coeffs(l), ref.coeff_array(V.smoother.c), what + (l, "coeffs"))
    assert s.interval() == s.interval(0)
    same(s.dinv(), op.to_orig(hier.dinv), what + ("dinv",))
    assert s.launches_per_body() == hier.launches_per_body(fused_dot(p, fmt, C)), what
    assert s.precond_bytes() == hier.bytes(), (what, s.precond_bytes(), hier.bytes())
    for l in range(hier.L - 1):
        V, W = hier.lev[l], hier.lev[l + 1]
        for seed, special in ((3, False), (4, True)):
            r, w, z, zc = (ref.probe_vector(V.n, seed, special), ref.probe_vector(V.n, seed + 5, special),
                           ref.probe_vector(V.n, seed + 10, special), ref.probe_vector(W.n, seed + 20, special))
            if special and V.n > 8:  # an inf in w beside rows that do not touch it, a NaN in zc
                w[5], zc[W.n // 2] = -np.inf, np.nan
            want = hier.probe_w(l, V.op.to_dev(r), V.op.to_dev(w), V.op.to_dev(z), W.op.to_dev(zc))
            got = s.mg_poly_probe(l, r, w, z, zc)
            for name, g, wv, o in zip(("rc", "z_out"), got, want, (W.op, V.op)):
                same(g, o.to_orig(wv), what + (l, name, "special" if special else "finite"))
    if cycles:
        for seed, special in ((1, False), (2, True)):
            r = ref.probe_vector(hier.n, seed, special)
            want = op.to_orig(hier.apply(op.to_dev(r))[0])
            same(s.apply(r), want, what + ("cycle", "special" if special else "finite"))
            if hier.n > 5:
                assert np.isnan(want).any() == special
        assert s.apply_ms(2) > 0.0


def check(matrix, levels, fmt, C, sigma, tmp, **kw):
    c = dict(matrix=matrix, fmt=fmt, C=C, sigma=sigma, levels=levels, **kw)
    hier, transfers = ref.build_hierarchy(ref.MGPOLY, c, tmp)
    assert hier.L == levels
    p = hostapi.Problem(*pcg_ref.problem_args(matrix, tmp), fmt=fmt, Cc=C, sigma=sigma)
    if sigma > 1:  # the restatement walks the device's own permutation
        op = hier.lev[0].op
        assert np.array_equal(p.array("oldToNewPerm"), op.o2n if op.o2n is not None else np.arange(p.nr))
    s = hostapi.PCG(p, precond="mgpoly", levels=levels, **kw)
    check_handle(s, p, hier, fmt, C, (matrix, levels, fmt, C, sigma))
    s.free(), p.free(), hier.free()
    return hier


@pytest.mark.parametrize("fmt,C,sigma", cases.KERNEL_FORMATS)
@pytest.mark.parametrize("matrix,levels", cases.KERNEL_SHAPES, ids=lambda m: "_".join(str(v) for v in m) if isinstance(m, tuple) else "L%d" % m)
def test_transfers_levels_and_one_cycle_equal_the_restatement(gpu, matrix, levels, fmt, C, sigma, tmp):
    hier = check(matrix, levels, fmt, C, sigma, tmp)
    rows = [V.n for V in hier.lev]
    if matrix == ("dims", 4, 4, 4):
        assert rows == [64, 8] and int(hier.lev[0].transfer.PT[0].max()) == 27  # one partial chunk of P^T; two batches of 16 in a row
    if matrix == ("dims", 16, 16, 16):
        assert rows == [4096, 512, 64, 8]
    c0 = hier.lev[0].smoother.c
    assert hier.lev[0].transfer.omega == 0.25 and hier.steps == hier.coarse_steps == 2 and c0["lmax"] / c0["lmin"] == 4.0


def test_sell_4_8(gpu, tmp):
    matrix, levels = cases.SELL_4_8_SHAPE
    check(matrix, levels, "scs", 4, 8, tmp)


@pytest.mark.parametrize("steps,coarse_steps", [(1, None), (2, None), (3, None), (3, 1), (1, 4)])
def test_one_cycle_per_step_count_in_both_kernel_modes(gpu, steps, coarse_steps, tmp):
    """16^3 at four levels in Sell-64-256: the row programs (mode 5) and the reference-layout stream (mode 0) on every level"""
    c = dict(matrix=("hpcg", 16), fmt="scs", C=64, sigma=256, levels=4, steps=steps, coarse_steps=coarse_steps)
    hier, transfers = ref.build_hierarchy(ref.MGPOLY, c, tmp)
    op = hier.lev[0].op
    p = hostapi.Problem("generate", 16, 16, 16, fmt="scs", Cc=64, sigma=256)
    seen = modes(p)
    assert seen == [5, 0], seen
    s = hostapi.PCG(p, precond="mgpoly", levels=4, steps=steps, coarse_steps=coarse_steps)
    assert s.launches_per_body() == 4 + 3 * (4 * steps + 2) + 2 * (coarse_steps or steps) - 1
    check_handle(s, p, hier, "scs", 64, (steps, coarse_steps), cycles=False)
    for mode in seen:
        assert p.use_packed(mode) == mode
        for seed, special in ((1, False), (2, True)):
            r = ref.probe_vector(hier.n, seed, special)
            same(s.apply(r), op.to_orig(hier.apply(op.to_dev(r))[0]), (steps, coarse_steps, mode, special))
    s.free(), p.free(), hier.free()


def test_a_callers_lmax_and_ratio_hold_on_every_level(gpu, tmp):
    kw = dict(steps=2, coarse_steps=3, lmax=1.75, ratio=8.0)
    hier = check(("dims", 8, 8, 8), 3, "scs", 64, 256, tmp, **kw)
    assert all(V.smoother.c["lmax"] == 1.75 and V.smoother.c["lmin"] == 1.75 / 8.0 for V in hier.lev)


@pytest.mark.parametrize("fmt,sigma", [("crs", 1), ("scs", 1), ("scs", 256)])
def test_a_callers_hierarchy_with_an_empty_row_and_a_zero_weight(gpu, fmt, sigma, tmp):
    fine, coarse, P, omega = cases.hand_made(tmp)
    outs = []
    for store_zero in (True, False):
        c = cases.hand_made_case(tmp, fmt, sigma, store_zero)
        hier, transfers = ref.build_hierarchy(ref.MGPOLY, c, tmp)
        P = transfers[0][0]
        assert [V.n for V in hier.lev] == [130, 65] and omega == 0.5 and (0.0 in P[2].tolist()) == store_zero
        assert (hier.lev[0].transfer.P[0] == 0).sum() == 1  # the empty row
        p = hostapi.Problem(fine, 1, 1, 1, fmt=fmt, Cc=64, sigma=sigma)
        q = hostapi.Problem(coarse, 1, 1, 1, fmt=fmt, Cc=64, sigma=sigma)
        s = hostapi.PCG(p, precond="mgpoly", coarse=[(q, P, omega)])
        check_handle(s, p, hier, fmt, 64, ("hand made", fmt, sigma, store_zero))
        # the empty row's z goes through the prolongation untouched, the sign of its zero included
        z = np.ones(130)
        z[cases.EMPTY_ROW] = -0.0
        zo = s.mg_poly_probe(0, np.zeros(130), np.zeros(130), z, np.zeros(65))[1]
        assert zo[cases.EMPTY_ROW] == 0.0 and np.signbit(zo[cases.EMPTY_ROW])
        outs.append(s.apply(ref.probe_vector(130, 9, True)))
        s.free(), q.free(), p.free(), hier.free()
    same(outs[0], outs[1], "a stored weight of 0.0 changes nothing")


def test_other_kinds_refuse_the_level_queries(gpu):
    p = hostapi.Problem("generate", 8, 8, 8, fmt="crs")
    j, q = hostapi.PCG(p), hostapi.PCG(p, precond="poly")
    with pytest.raises(ValueError, match="not 'poly'"):
        j.interval(0)
    with pytest.raises(ValueError, match="a level goes with precond='mgpoly' only"):
        q.coeffs(0)
    m = hostapi.PCG(p, precond="mgpoly", levels=2)
    with pytest.raises(ValueError, match="level 2 of a handle with 2 levels"):
        m.interval(2)
    with pytest.raises(ValueError, match="not 'poly'"):
        m.rowbound()
    m.free(), q.free(), j.free(), p.free()
