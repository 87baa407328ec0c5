"""The two vector kernels of GMRES on their own (sb_multidot, sb_multiaxpy_sub) against the two loops of the CPU
restatement (tests/gmres_ref.py: multidot, multiaxpy_sub) BIT FOR BIT, and the device's sqrt and / against numpy."""
import numpy as np
import pytest

import gmres_ref
from sparsebench_amd import capi

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 255, 256, 257, 1430, 4096, 100003]
NVECS = [1, 2, 3, 4, 5, 8, 31]


def bits_equal(a, b):
    """same bit patterns; where one side is NaN the other must be NaN too (NaN payloads and signs are not compared)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


def make(n, nvec, kind, seed):
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((nvec, n))
    w = rng.standard_normal(n)
    h = rng.standard_normal(nvec)
    tiny = np.float64(5e-324)
    if kind == "finite":  # -0.0, subnormals, large and small magnitudes: every result stays finite
        for arr in (V.reshape(-1), w):
            k = max(1, arr.size // 7)
            idx = rng.integers(0, arr.size, k)
            arr[idx] = rng.choice(np.array([-0.0, 0.0, tiny, -tiny, 2.2e-308, -1.1e-308, 1e150, -1e150, 1e-150]), k)
    elif kind == "nonfinite":  # rows holding NaN and +-Inf
        for arr in (V.reshape(-1), w):
            k = max(1, arr.size // 50)
            idx = rng.integers(0, arr.size, k)
            arr[idx] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, tiny]), k)
        if nvec > 2:
            h[1] = np.inf
    return V, w, h


def upload(V, ldv):
    nvec, n = V.shape
    host = np.full((nvec, ldv), np.nan)  # the padding behind n is never read: NaN there must not show
    host[:, :n] = V
    return capi.DeviceVector.from_host(host.reshape(-1))


@pytest.mark.parametrize("kind", ["random", "finite", "nonfinite"])
@pytest.mark.parametrize("n", NS)
def test_multidot_and_multiaxpy_sub_bit_for_bit(gpu, n, kind):
    L = gpu
    for nvec in NVECS:
        V, w, h = make(n, nvec, kind, 1000 * n + nvec)
        ldv = ((n + 1) // 2) * 2 + 6
        dV, dw = upload(V, ldv), capi.DeviceVector.from_host(w)
        dh = capi.DeviceVector(nvec)
        L.sb_multidot(n, nvec, dV.ptr, ldv, dw.ptr, dh.ptr)
        got = dh.get()
        want = np.array(gmres_ref.multidot(list(V), w))
        assert bits_equal(got, want), (n, nvec, kind, got, want)
        # the projections: the h of the dots where finite (as the solver uses them), random coefficients otherwise
        c = got if np.all(np.isfinite(got)) and kind != "nonfinite" else h
        dc = capi.DeviceVector.from_host(c)
        L.sb_multiaxpy_sub(n, nvec, dV.ptr, ldv, dc.ptr, dw.ptr)
        wn = dw.get()
        assert bits_equal(wn, gmres_ref.multiaxpy_sub(list(V), c, w)), (n, nvec, kind)
        assert bits_equal(dV.get().reshape(nvec, ldv)[:, :n], V)  # V untouched
        for d in (dV, dw, dh, dc):
            d.free()


def second_trip_n(L):
    """gm_multidot_k / gm_multiupdate_k: a wave per 256-row group, four waves per workgroup; one full group more than the capped
    grid has waves, then 257 rows -- from the launch the library reports"""
    out = np.zeros(3, dtype=np.uint32)
    L.sb_gmres_group_launch(0x7FFFFF00, out.ctypes.data)
    cap, threads, cus = int(out[0]), int(out[1]), int(out[2])
    assert threads == 256 and cap >= cus >= 1
    n = 256 * (cap * 4) + 257
    L.sb_gmres_group_launch(n, out.ctypes.data)
    assert int(out[0]) == cap  # the grid is at its cap: the groups `4 cap` and `4 cap + 1` are second trips, the last one partial
    return n


@pytest.mark.parametrize("nvec", [1, 5])
@pytest.mark.parametrize("kind", ["random", "nonfinite"])
def test_second_grid_stride_trip_bit_for_bit(gpu, kind, nvec):
    """both kernels past the grid's cap, under and past the multidot's unroll"""
    L = gpu
    n = second_trip_n(L)
    print("second grid-stride trip with a partial last group at n =", n)
    V, w, h = make(n, nvec, kind, 77 * nvec + len(kind))
    ldv = ((n + 1) // 2) * 2 + 6
    dV, dw, dh = upload(V, ldv), capi.DeviceVector.from_host(w), capi.DeviceVector(nvec)
    L.sb_multidot(n, nvec, dV.ptr, ldv, dw.ptr, dh.ptr)
    got = dh.get()
    want = np.array(gmres_ref.multidot(list(V), w))
    assert bits_equal(got, want), (n, nvec, kind, got, want)
    c = got if np.all(np.isfinite(got)) and kind != "nonfinite" else h
    dc = capi.DeviceVector.from_host(c)
    L.sb_multiaxpy_sub(n, nvec, dV.ptr, ldv, dc.ptr, dw.ptr)
    assert bits_equal(dw.get(), gmres_ref.multiaxpy_sub(list(V), c, w)), (n, nvec, kind)
    assert bits_equal(dV.get().reshape(nvec, ldv)[:, :n], V)  # V untouched
    for d in (dV, dw, dh, dc):
        d.free()


def test_device_sqrt_and_divide_are_correctly_rounded(gpu):
    L = gpu
    rng = np.random.default_rng(7)
    a = np.concatenate([np.exp(rng.uniform(-700, 700, 5000)), rng.standard_normal(2500) ** 2, rng.uniform(0, 4, 2500),
                        [0.0, -0.0, np.inf, np.nan, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 1.0, 2.0, 3.0, -1.0]])
    b = np.concatenate([rng.standard_normal(5000) * np.exp(rng.uniform(-300, 300, 5000)), rng.uniform(0.5, 2, 5000),
                        [1.0, 3.0, np.inf, 1.0, 3.0, 7.0, 0.1, 3.0, 3.0, 0.0, 5e-324]])
    assert len(a) == len(b) >= 10000
    da, db = capi.DeviceVector.from_host(a), capi.DeviceVector.from_host(b)
    ds, dd = capi.DeviceVector(len(a)), capi.DeviceVector(len(a))
    L.sb_debug_sqrt_div(len(a), da.ptr, db.ptr, ds.ptr, dd.ptr)
    with np.errstate(all="ignore"):
        assert bits_equal(ds.get(), np.sqrt(a))
        assert bits_equal(dd.get(), a / b)
    for d in (da, db, ds, dd):
        d.free()
