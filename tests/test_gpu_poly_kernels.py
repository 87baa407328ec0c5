"""The kernels of the Chebyshev polynomial preconditioner alone, BIT FOR BIT against the CPU restatement
(tests/precond_ref.py, pinned by tests/test_poly_host.py), NaN equal to NaN: the r update with step 1 and the step kernel through
their native entries at the sizes where their paths change -- fewer rows than one wave's span, the partial last group, an odd n,
every wave on a second trip of its group loop -- with +0.0, -0.0, denormals, an inf and a NaN in every vector and guard doubles
behind them; the bound's row values, the coefficients and the interval in every format; and one apply through
sb_pcg_apply_precond for steps 1 .. 4 in both kernel modes of the SpMV."""
import numpy as np
import pytest

from oracle import pyoracle as po

import pcg_ref
import poly_cases
import precond_ref as ref
from sparsebench_amd import hostapi
from sparsebench_amd.capi import DeviceVector

pytestmark = pytest.mark.gpu
GUARD = 9.9


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("poly_kernels")


def same(got, want, what):
    a, b = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), (what, "NaN positions differ", np.nonzero(na != nb)[0][:5])
    bad = np.nonzero((a.view(np.uint64) != b.view(np.uint64)) & ~na)[0]
    assert bad.size == 0, (what, "first difference at", int(bad[0]), a[bad[0]], b[bad[0]], "of", bad.size)


def vectors(n, seed, count):
    """`count` vectors of precond_ref.probe_vector(special=True), each rolled by its own offset so that the special values of
    different vectors meet ordinary ones; dinv-like vectors are used as they come (the kernels do not ask for positive ones)"""
    return [np.roll(ref.probe_vector(n, seed + 31 * w, special=True), 5 * w) for w in range(count)]


def guarded(v, extra=4):
    return DeviceVector.from_host(np.concatenate((v, np.full(extra, GUARD))))


def check_guarded(dv, want, what):
    got = dv.get()
    same(got[:len(want)], want, what)
    assert np.all(got[len(want):] == GUARD), (what, "guard doubles were written")


def two_trips_n(L):
    """the smallest n with a partial, odd last group at which EVERY wave of the launch makes at least two trips of its group
    loop: twice as many full groups as the grid at its cap has waves, then 257 rows -- from the launch the library reports"""
    out = np.zeros(3, dtype=np.uint32)
    L.sb_pcg_poly_step_launch(0x7FFFFF00, out.ctypes.data)
    cap, threads, cus = int(out[0]), int(out[1]), int(out[2])
    assert threads == 1024 and cap >= cus >= 1
    waves = cap * (threads // 64)
    n = 256 * 2 * waves + 257
    L.sb_pcg_poly_step_launch(n, out.ctypes.data)
    assert int(out[0]) == cap
    return n


SIZES = poly_cases.KERNEL_N + ["two_trips"]


@pytest.mark.parametrize("n", SIZES)
def test_update_r_native_equals_the_restatement(gpu, n):
    L = gpu
    if n == "two_trips":
        n = two_trips_n(L)
        print("every wave makes two trips at n =", n)
    r, Ap, dinv = vectors(n, seed=n % 1000, count=3)
    nalpha, c1 = -0.37109375, 0.94140625
    nG = (n + 255) // 256
    for pro in (0, 1):
        want_r, want_z, want_l1rz, want_l1rr = ref.update_r(r, Ap, dinv, -1.0 if pro else nalpha, c1)
        assert len(want_l1rz) == len(want_l1rr) == nG
        for last in (0, 1):
            what = (n, "pro", pro, "last", last)
            dr, dA, di = guarded(r), guarded(Ap), guarded(dinv)
            dd, dz = guarded(np.full(n, 7.7)), guarded(np.full(n, 7.7))
            dlz, dlr = DeviceVector.from_host(np.full(nG + 4, GUARD)), DeviceVector.from_host(np.full(nG + 4, GUARD))
            L.sb_pcg_poly_update_r_native(n, pro, last, nalpha, c1, dA.ptr, dr.ptr, di.ptr, dd.ptr, dz.ptr, dlz.ptr, dlr.ptr)
            check_guarded(dr, want_r, what + ("r",))
            check_guarded(dd, want_z, what + ("d",))
            check_guarded(dz, want_z, what + ("z",))
            check_guarded(dA, Ap, what + ("Ap untouched",))
            check_guarded(di, dinv, what + ("dinv untouched",))
            check_guarded(dlr, want_l1rr, what + ("level-1 r.r",))
            check_guarded(dlz, want_l1rz if last else np.zeros(0), what + ("level-1 r.z",))
            for v in (dr, dA, di, dd, dz, dlz, dlr):
                v.free()


@pytest.mark.parametrize("n", SIZES)
def test_step_native_equals_the_restatement(gpu, n):
    L = gpu
    if n == "two_trips":
        n = two_trips_n(L)
    r, w, dinv, d, z = vectors(n, seed=(n + 7) % 1000, count=5)
    a, b = 0.1708984375, 0.7294921875
    nG = (n + 255) // 256
    want_d, want_z, want_l1 = ref.step_l1(r, w, dinv, d, z, a, b)
    assert len(want_l1) == nG
    if n > 5:
        assert np.isnan(want_z).any()  # the special values reach the result
    for last in (0, 1):
        what = (n, "last", last)
        dr, dw, di, dd, dz = guarded(r), guarded(w), guarded(dinv), guarded(d), guarded(z)
        dl = DeviceVector.from_host(np.full(nG + 4, GUARD))
        L.sb_pcg_poly_step_native(n, last, a, b, dr.ptr, dw.ptr, di.ptr, dd.ptr, dz.ptr, dl.ptr)
        check_guarded(dd, want_d, what + ("d",))
        check_guarded(dz, want_z, what + ("z",))
        check_guarded(dr, r, what + ("r untouched",))
        check_guarded(dw, w, what + ("w untouched",))
        check_guarded(di, dinv, what + ("dinv untouched",))
        check_guarded(dl, want_l1 if last else np.zeros(0), what + ("level-1 r.z",))
        for v in (dr, dw, di, dd, dz, dl):
            v.free()


def test_kernels_on_clean_data_give_the_tree_dots(gpu):
    n = 5000
    rng = np.random.default_rng(3)
    r, Ap, dinv = rng.standard_normal(n), rng.standard_normal(n), 1.0 + rng.random(n)
    want_r, want_z, l1rz, l1rr = ref.update_r(r, Ap, dinv, 0.25, 0.5)
    assert po.reduce_final(l1rz) == po.ddot_tree(want_r, want_z) and np.isfinite(po.reduce_final(l1rr))
    nG = (n + 255) // 256
    dr, dA, di, dd, dz = (DeviceVector.from_host(v) for v in (r, Ap, dinv, np.zeros(n), np.zeros(n)))
    dlz, dlr = DeviceVector(nG), DeviceVector(nG)
    gpu.sb_pcg_poly_update_r_native(n, 0, 1, 0.25, 0.5, dA.ptr, dr.ptr, di.ptr, dd.ptr, dz.ptr, dlz.ptr, dlr.ptr)
    same(dlz.get(), l1rz, "level-1 r.z")
    same(dlr.get(), l1rr, "level-1 r.r")
    for v in (dr, dA, di, dd, dz, dlz, dlr):
        v.free()


def modes(p):
    """the kernel modes the matrix has: 5 (masked row programs) where it has them, and 0 (the reference-layout stream)"""
    return sorted({p.use_packed(5), p.use_packed(0)}, reverse=True)


@pytest.mark.parametrize("fmt,C,sigma", poly_cases.APPLY_FORMATS)
@pytest.mark.parametrize("matrix", poly_cases.APPLY_MATRICES, ids=lambda m: "_".join(str(v) for v in m))
def test_rowbound_coefficients_and_apply_equal_the_restatement(gpu, matrix, fmt, C, sigma, tmp):
    g = pcg_ref.gmatrix(matrix, tmp)
    op = pcg_ref.operator(g, fmt, C, sigma)
    p = hostapi.Problem(*pcg_ref.problem_args(matrix, tmp), fmt=fmt, Cc=C, sigma=sigma)
    if sigma > 1:  # the restatement walks the device's own permutation
        assert np.array_equal(p.array("oldToNewPerm"), op.o2n if op.o2n is not None else np.arange(p.nr))
    what = (matrix, fmt, C, sigma)
    seen = modes(p)
    if matrix[0] == "hpcg":
        assert seen[0] == 5 or C != 64, seen
    probes = [ref.probe_vector(g.nr, 1, False), ref.probe_vector(g.nr, 2, True)]
    for steps in (1, 2, 3, 4):
        plan = ref.poly(g, op, steps=steps)
        ch = plan.lev[0].smoother
        s = hostapi.PCG(p, precond="poly", steps=steps)
        assert s.precond() == "poly" and s.steps() == steps and s.colours() == 0 and s.levels() == 0
        same(s.dinv(), op.to_orig(plan.dinv), what + ("dinv",))
        same(s.rowbound(), op.to_orig(ch.g), what + ("rowbound",))
        assert s.interval() == (ch.c["lmin"], ch.c["lmax"]) and ch.c["lmax"] == np.max(ch.g)
        same(s.coeffs(), ref.coeff_array(ch.c), what + ("coeffs", steps))
        for mode in seen:
            assert p.use_packed(mode) == mode
            for r, special in zip(probes, (False, True)):
                want = op.to_orig(plan.apply(op.to_dev(r))[0])
                same(s.apply(r), want, what + (steps, mode, "special" if special else "finite"))
                assert np.isnan(want).any() == special
        assert s.precond_bytes() == (steps - 1) * (gpu.sb_matrix_spmv_bytes(p.matrix) + 56.0 * g.nr) + 24.0 * g.nr
        assert s.apply_ms(2) > 0.0
        s.free()
    p.free(), g.free()


@pytest.mark.parametrize("steps,lmax,ratio", [(16, None, None), (1, 1.6, 4.0), (4, 1.37, 30.0), (3, 2.5, 8.0), (2, None, 4.0)])
def test_coefficients_and_interval_for_a_callers_arguments(gpu, steps, lmax, ratio, tmp):
    matrix = ("scaled", 8)
    g = pcg_ref.gmatrix(matrix, tmp)
    op = pcg_ref.operator(g, "scs", 64, 256)
    p = hostapi.Problem(*pcg_ref.problem_args(matrix, tmp), fmt="scs", Cc=64, sigma=256)
    plan = ref.poly(g, op, steps=steps, lmax=lmax, ratio=ref.RATIO[ref.POLY] if ratio is None else ratio)
    ch = plan.lev[0].smoother
    s = hostapi.PCG(p, precond="poly", steps=steps, lmax=lmax, ratio=ratio)
    assert s.steps() == steps and s.interval() == (ch.c["lmin"], ch.c["lmax"])
    if lmax is not None:
        assert s.interval()[1] == lmax
    same(s.coeffs(), ref.coeff_array(ch.c), (steps, lmax, ratio))
    assert len(s.coeffs()) == 2 * steps - 1
    same(s.rowbound(), op.to_orig(ch.g), "rowbound")  # computed whoever supplies lmax
    r = ref.probe_vector(g.nr, 4, False)
    same(s.apply(r), op.to_orig(plan.apply(op.to_dev(r))[0]), ("apply", steps, lmax, ratio))
    s.free(), p.free(), g.free()


def test_other_kinds_report_no_steps_and_refuse_the_queries(gpu):
    p = hostapi.Problem("generate", 8, 8, 8, fmt="crs")
    j = hostapi.PCG(p)
    assert j.steps() == 0 and j.precond() == "jacobi"
    for name in ("interval", "coeffs", "rowbound"):
        with pytest.raises(ValueError, match="not 'poly'"):
            getattr(j, name)()
    j.free(), p.free()
