"""The two update kernels of BiCGStab under a preconditioner plan alone, through their blocking native entries, BIT
FOR BIT against the restatement's elementwise forms (bicgstab_ref.update_p / update_s, and for CHEB = 1 the first Chebyshev step
(p o dinv) * c1 on top, precond_ref's `Cheb.pre` arithmetic): at the eleven sizes of test_gpu_bicgstab_kernels.sizes(), both CHEB
values, with NaN, +-Inf, -0.0 and subnormals at distinct positions of distinct inputs, every vector between sentinels, every input
that is not an output untouched."""
import numpy as np
import pytest

import bicgstab_precond_ref as pref
import bicgstab_ref as ref
from test_gpu_bicgstab_kernels import N_SIZES, SENTINEL, Guarded, same, sizes, specials

pytestmark = pytest.mark.gpu
C1 = 0.3173828125  # (any finite double: the kernels take it by value)


@pytest.fixture(scope="module")
def ns(gpu):
    s = sizes(gpu)
    assert len(s) == N_SIZES
    return s


def run_p(gpu, n, cheb, r, p, v, dinv, beta, omega):
    want_p = ref.update_p(r, p, v, dinv, beta, omega)[0]
    dr, dp, dv, dd = Guarded(r), Guarded(p), Guarded(v), Guarded(dinv)
    d_d, d_h = Guarded(n=n), Guarded(n=n)
    if cheb:
        gpu.sb_bicgstab_plan_update_p_native(n, 1, C1, beta, omega, dr.ptr, dp.ptr, dv.ptr, dd.ptr, d_d.ptr, d_h.ptr)
    else:
        gpu.sb_bicgstab_plan_update_p_native(n, 0, C1, beta, omega, dr.ptr, dp.ptr, dv.ptr, None, None, None)
    same(dp.get("p"), want_p, (n, cheb, "p"))
    if cheb:
        want_d = pref.plan_update(want_p, dinv, C1)
        same(d_d.get("d"), want_d, (n, "d"))
        same(d_h.get("ph"), want_d, (n, "ph"))
    else:  # the sweeps make ph from zero: the kernel writes p alone
        assert np.all(d_d.get("d") == SENTINEL) and np.all(d_h.get("ph") == SENTINEL)
    for d, a, w in ((dr, r, "r"), (dv, v, "v"), (dd, dinv, "dinv")):
        same(d.get(w), a, (n, cheb, w, "untouched"))
    for d in (dr, dp, dv, dd, d_d, d_h):
        d.free()


@pytest.mark.parametrize("cheb", [0, 1])
@pytest.mark.parametrize("i", range(N_SIZES))
def test_plan_update_p(gpu, ns, i, cheb):
    n = ns[i]
    r, p, v, dinv = specials(n, 500 + i, 4)
    run_p(gpu, n, cheb, r, p, v, dinv, -0.37109375, 1.2890625)


@pytest.mark.parametrize("cheb", [0, 1])
def test_plan_update_p_first_body_form(gpu, cheb):
    """beta = omega = 0.0 on zeroed p and v: p = r + 0.0 (so -0.0 becomes +0.0), whatever r holds"""
    n = 777
    r, dinv = specials(n, 17, 2)
    run_p(gpu, n, cheb, r, np.zeros(n), np.zeros(n), dinv, 0.0, 0.0)


@pytest.mark.parametrize("cheb", [0, 1])
@pytest.mark.parametrize("i", range(N_SIZES))
def test_plan_update_s(gpu, ns, i, cheb):
    n = ns[i]
    r, v, dinv = specials(n, 600 + i, 3)
    alpha = 0.8203125
    want_s = ref.update_s(r, v, dinv, alpha)[0]
    inplace = i % 2 == 0  # the loop keeps s in r's storage
    dr, dv, dd = Guarded(r), Guarded(v), Guarded(dinv)
    d_d, d_h = Guarded(n=n), Guarded(n=n)
    ds = dr if inplace else Guarded(n=n)
    if cheb:
        gpu.sb_bicgstab_plan_update_s_native(n, 1, C1, alpha, dr.ptr, dv.ptr, dd.ptr, ds.ptr, d_d.ptr, d_h.ptr)
    else:
        gpu.sb_bicgstab_plan_update_s_native(n, 0, C1, alpha, dr.ptr, dv.ptr, None, ds.ptr, None, None)
    same(ds.get("s"), want_s, (n, cheb, "s"))
    if cheb:
        want_d = pref.plan_update(want_s, dinv, C1)
        same(d_d.get("d"), want_d, (n, "d"))
        same(d_h.get("sh"), want_d, (n, "sh"))
    else:
        assert np.all(d_d.get("d") == SENTINEL) and np.all(d_h.get("sh") == SENTINEL)
    if not inplace:
        same(dr.get("r"), r, (n, "r untouched"))
        ds.free()
    same(dv.get("v"), v, (n, "v untouched"))
    same(dd.get("dinv"), dinv, (n, "dinv untouched"))
    for d in (dr, dv, dd, d_d, d_h):
        d.free()

