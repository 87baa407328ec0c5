"""The three kernels of right-preconditioned GMRES that write the first part of M^-1 of the vector they make, each
alone through its blocking native entry, BIT FOR BIT against the restatement's formula (gmres_precond_ref.first: v o dinv for a
diagonal, (v o dinv) * c1 for the Chebyshev plans, c1 from a real plan) and against the unfused twin it stands in for (mode -1 of
the same entry: V, x, H's column, g and the estimate are the twin's bits).  Sizes around the 256-row group and the two-element
tail, off every grid (1 430, 4 099); +-0.0, subnormals, +-Inf and NaN at distinct positions of the vector and of dinv; every
output between sentinels, every input that is not an output untouched."""
import math

import numpy as np
import pytest

from oracle import pyoracle as po

import gmres_precond_cases as cases
import gmres_precond_ref as ref
import gmres_ref
from sparsebench_amd.capi import DeviceVector
from test_gpu_bicgstab_kernels import SENTINEL, Guarded, same, specials

pytestmark = pytest.mark.gpu
NS = [1, 2, 255, 256, 257, 511, 513, 1430, 4099]


@pytest.fixture(scope="module")
def c1(tmp_path_factory):
    plan = ref.build_plan(cases.CASES["cd16_crs_poly_3_16_m30"], tmp_path_factory.mktemp("gmres_precond_kernels"))[0]
    v = float(plan.lev[0].smoother.c["c1"])
    plan.free()
    assert 0.0 < v < 10.0 and math.isfinite(v)
    return v


def check_rider(mode, c1, v, dinv, d_d, d_z, what):
    want = ref.first(v, dinv, c1 if mode else None)
    same(d_z.get("z"), want, what + ("z",))
    if mode:
        same(d_d.get("d"), want, what + ("d",))
    else:  # a diagonal has no recurrence: d is not touched
        assert np.all(d_d.get("d") == SENTINEL), what


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_scale_with_the_first_part(gpu, n, mode, c1):
    a, dinv = specials(n, 700 + n, 2)
    for scalar in (1.7109375, -3.0e-5):
        want = a / np.float64(scalar)
        ds = DeviceVector.from_host(np.array([scalar, SENTINEL]))
        dg = DeviceVector.from_host(np.array([SENTINEL, SENTINEL]))
        da, dd, d_out, d_d, d_z, d_twin = Guarded(a), Guarded(dinv), Guarded(n=n), Guarded(n=n), Guarded(n=n), Guarded(n=n)
        gpu.sb_gmres_pre_scale_native(n, mode, c1, da.ptr, ds.ptr, d_out.ptr, dg.ptr, dd.ptr, d_d.ptr, d_z.ptr)
        out = d_out.get("out")
        same(out, want, (n, mode, "out"))
        assert np.array_equal(dg.get(), [scalar, SENTINEL])
        check_rider(mode, c1, out, dinv, d_d, d_z, (n, mode, scalar))
        dg.set(np.array([SENTINEL, SENTINEL]))
        gpu.sb_gmres_pre_scale_native(n, -1, 0.0, da.ptr, ds.ptr, d_twin.ptr, dg.ptr, None, None, None)
        same(d_twin.get("twin"), out, (n, mode, "the twin's out"))
        assert np.array_equal(dg.get(), [scalar, SENTINEL])
        same(da.get("a"), a, (n, "a untouched")), same(dd.get("dinv"), dinv, (n, "dinv untouched"))
        for d in (ds, dg, da, dd, d_out, d_d, d_z, d_twin):
            d.free()


def basis(n, nvec, seed):
    V = np.stack(specials(n, seed, nvec))
    ldv = ((n + 1) // 2) * 2 + 6
    host = np.full((nvec, ldv), np.nan)  # the padding behind n is never read: NaN there must not show
    host[:, :n] = V
    return V, ldv, DeviceVector.from_host(host.reshape(-1))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_x_update_with_the_first_part(gpu, n, mode, c1):
    for nvec in (1, 4, 7):  # below, at and past the unroll of 4
        V, ldv, dV = basis(n, nvec, 800 + 10 * n + nvec)
        x, dinv = specials(n, 900 + n + nvec, 2)
        y = np.random.default_rng(n + nvec).standard_normal(nvec)
        with np.errstate(all="ignore"):
            want = np.array(x)
            for i in range(nvec):
                want = want + np.float64(y[i]) * V[i]  # gmres_ref.solve's x update
        dy = DeviceVector.from_host(y)
        dx, dd, d_d, d_z, d_twin = Guarded(x), Guarded(dinv), Guarded(n=n), Guarded(n=n), Guarded(x)
        gpu.sb_gmres_pre_multiupdate_native(n, mode, c1, nvec, dV.ptr, ldv, dy.ptr, dx.ptr, dd.ptr, d_d.ptr, d_z.ptr)
        xn = dx.get("x")
        same(xn, want, (n, mode, nvec, "x"))
        check_rider(mode, c1, xn, dinv, d_d, d_z, (n, mode, nvec))
        gpu.sb_gmres_pre_multiupdate_native(n, -1, 0.0, nvec, dV.ptr, ldv, dy.ptr, d_twin.ptr, None, None, None)
        same(d_twin.get("twin"), xn, (n, mode, nvec, "the twin's x"))
        same(dd.get("dinv"), dinv, (n, "dinv untouched"))
        same(dV.get().reshape(nvec, ldv)[:, :n], V, (n, "V untouched"))
        for d in (dV, dy, dx, dd, d_d, d_z, d_twin):
            d.free()


def finite_specials(n, seed):
    """+-0.0, subnormals and wide magnitudes at distinct positions: w . w stays finite and positive"""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(n) + 0.25
    tiny = np.float64(5e-324)
    for j, val in enumerate([-0.0, 0.0, tiny, -tiny, 1e-310, 1e-160, -1e100]):
        if n > 1:
            w[(5 * j + 1) % n] = val
    w[0] = 1.5
    return w


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_step_and_normalise_with_the_first_part(gpu, n, mode, c1):
    dinv = specials(n, 1000 + n, 1)[0]
    for j, w in ((0, finite_specials(n, 1100 + n)), (2, finite_specials(n, 1200 + n)), (1, specials(n, 1300 + n, 1)[0])):
        hcol = np.array([0.75, -1.25, 2.5][:j + 1])
        gj = 3.0
        wc = np.ascontiguousarray(w)
        with np.errstate(all="ignore"):
            l1 = po.ddot_partials(wc, wc)
            hn = np.sqrt(np.float64(po.ddot_tree(wc, wc)))
            want_v = w / hn
        assert len(l1) == (n + 255) // 256
        dl = DeviceVector.from_host(l1)
        outs = []
        for md in (mode, -1):
            dw, dd, d_v, d_d, d_z = Guarded(w), Guarded(dinv), Guarded(n=n), Guarded(n=n), Guarded(n=n)
            out = np.full(j + 1 + 6, SENTINEL)
            args = (dd.ptr, d_d.ptr, d_z.ptr) if md >= 0 else (None, None, None)
            gpu.sb_gmres_pre_step_native(n, md, c1, j, hcol.ctypes.data, gj, dl.ptr, dw.ptr, d_v.ptr, *args, out.ctypes.data)
            v = d_v.get("vnext")
            same(v, want_v, (n, md, j, "vnext"))
            same(out[-1:], [hn], (n, md, j, "hn"))
            if md >= 0:
                check_rider(md, c1, v, dinv, d_d, d_z, (n, md, j))
            else:
                assert np.all(d_d.get("d") == SENTINEL) and np.all(d_z.get("z") == SENTINEL)
            same(dw.get("w"), w, (n, "w untouched")), same(dd.get("dinv"), dinv, (n, "dinv untouched"))
            outs.append((out, v))
            for d in (dw, dd, d_v, d_d, d_z):
                d.free()
        same(outs[0][0], outs[1][0], (n, mode, j, "H's column, cs, sn, g[j], g[j+1], the estimate, hn: the twin's"))
        same(outs[0][1], outs[1][1], (n, mode, j, "V[j+1]: the twin's"))
        out = outs[0][0]
        same(out[j + 5:j + 6], np.abs(out[j + 4:j + 5]), (n, mode, j, "the estimate is |g[j+1]|"))
        if np.isfinite(hn):  # the scalar step itself, as gmres_ref.solve takes it at a first column
            if j == 0:
                assert hn > 0.0 and np.isfinite(out).all()
                d = gmres_ref._sqrt(hcol[0] * hcol[0] + float(hn) * float(hn))
                cs, sn = gmres_ref._div(hcol[0], d), gmres_ref._div(float(hn), d)
                same(out, [d, cs, sn, cs * gj, -(sn * gj), abs(sn * gj), hn], (n, mode, "the first column's rotation"))
        dl.free()
