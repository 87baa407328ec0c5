"""The kernels of PCG alone, BIT FOR BIT against the CPU restatement (tests/pcg_ref.py): the diagonal of every
format in the device's row order, and the fused r update (r, z, both level-1 arrays) at the sizes where its paths change --
one lane, one span, the partial last group, an odd n, more groups than waves -- with NaN, +-Inf, -0.0 and subnormals in r, Ap
and dinv at distinct positions."""
import numpy as np
import pytest

from oracle import pyoracle as po

import pcg_cases
import pcg_ref as ref
from sparsebench_amd import hostapi
from sparsebench_amd.capi import DeviceVector

pytestmark = pytest.mark.gpu

SHAPES = {"hpcg8": ("hpcg", 8), "hpcg16": ("hpcg", 16), "hpcg_10_11_13": ("dims", 10, 11, 13), "band_klein": ("file", pcg_cases.BAND_KLEIN),
          "irregular12": ("irregular", 12), "scaled16": ("scaled", 16)}
FORMATS = {"crs": ("crs", 64, 1), "sell_64_1": ("scs", 64, 1), "sell_64_256": ("scs", 64, 256), "sell_4_8": ("scs", 4, 8)}


def same(got, want, what):
    a, b = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), (what, "NaN positions differ", np.nonzero(na != nb)[0][:5])
    bad = np.nonzero((a.view(np.uint64) != b.view(np.uint64)) & ~na)[0]
    assert bad.size == 0, (what, "first difference at", int(bad[0]), a[bad[0]], b[bad[0]])


@pytest.fixture(scope="module")
def matrices(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pcg_kernels")
    cache = {}

    def get(shape):
        if shape not in cache:
            g = ref.gmatrix(SHAPES[shape], tmp)
            cache[shape] = (g, ref.diagonal(g), ref.problem_args(SHAPES[shape], tmp))
        return cache[shape]

    return get


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_matrix_diagonal_equals_the_storage_order_rule(gpu, matrices, shape, fmt):
    g, d_orig, args = matrices(shape)
    f, Cc, sigma = FORMATS[fmt]
    p = hostapi.Problem(*args, fmt=f, Cc=Cc, sigma=sigma)
    op = ref.operator(g, f, Cc, sigma)
    if sigma > 1:
        assert np.array_equal(p.array("oldToNewPerm"), op.o2n if op.o2n is not None else np.arange(p.nr))
    dd = DeviceVector.from_host(np.full(p.nr + 4, 9.9))
    gpu.sb_matrix_diagonal(p.matrix, dd.ptr)
    got = dd.get()
    same(got[:p.nr], op.to_dev(d_orig), (shape, fmt))
    assert np.all(got[p.nr:] == 9.9)
    assert np.all(d_orig > 0.0) and np.all(np.isfinite(d_orig))
    dd.free(), p.free()


def specials(n, seed):
    """r, Ap, dinv: random, with the special values at distinct positions of distinct vectors"""
    rng = np.random.default_rng(seed)
    v = [rng.standard_normal(n), rng.standard_normal(n), np.exp2(rng.integers(-3, 4, n).astype(np.float64)) * (1.0 + rng.random(n))]
    tiny = np.float64(5e-324)
    kinds = [np.nan, np.inf, -np.inf, -0.0, tiny, -tiny, 1e-310]
    for j, val in enumerate(kinds):
        for w in range(3):  # kind j of vector w
            for pos in {(11 * j + 3 * w + 1) % n, (n // 2 + 7 * j + w) % n, (n - 1 - 3 * j - w) % n}:
                v[w][pos] = val
    return v


def second_trip_n(L):
    """the smallest n at which the launch makes a second grid-stride trip that ends in a partial (and odd) last group: one
    full group more than the grid has waves, then 257 rows -- from the launch configuration the library reports"""
    out = (np.zeros(3, dtype=np.uint32))
    L.sb_pcg_update_r_launch(0x7FFFFF00, out.ctypes.data)
    cap, threads, cus = int(out[0]), int(out[1]), int(out[2])
    assert threads == 1024 and cap >= cus >= 1
    waves = cap * (threads // 64)
    n = 256 * waves + 257
    L.sb_pcg_update_r_launch(n, out.ctypes.data)
    assert int(out[0]) == cap  # the grid is at its cap: group `waves` and the partial group `waves + 1` are second trips
    return n


SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 4097, 100003, "second_trip"]


@pytest.mark.parametrize("n", SIZES)
def test_update_r_native_equals_the_restatement(gpu, n):
    L = gpu
    if n == "second_trip":
        n = second_trip_n(L)
        print("second grid-stride trip with a partial last group at n =", n)
    r, Ap, dinv = specials(n, seed=n)
    nalpha = -0.37109375
    want_r, want_z, want_l1rz, want_l1rr, want_rz, want_rr = ref.update_r(r, Ap, dinv, nalpha)
    nG = (n + 255) // 256
    assert len(want_l1rz) == len(want_l1rr) == nG
    dr, dA, dd = DeviceVector.from_host(r), DeviceVector.from_host(Ap), DeviceVector.from_host(dinv)
    dz = DeviceVector.from_host(np.full(n + 2, 9.9))
    dlz, dlr = DeviceVector.from_host(np.full(nG + 4, 9.9)), DeviceVector.from_host(np.full(nG + 4, 9.9))
    L.sb_pcg_update_r_native(n, nalpha, dA.ptr, dr.ptr, dd.ptr, dz.ptr, dlz.ptr, dlr.ptr)
    same(dr.get(), want_r, (n, "r"))
    z = dz.get()
    same(z[:n], want_z, (n, "z"))
    assert np.all(z[n:] == 9.9)
    lz, lr = dlz.get(), dlr.get()
    assert np.all(lz[nG:] == 9.9) and np.all(lr[nG:] == 9.9)
    same(lz[:nG], want_l1rz, (n, "level-1 r.z"))
    same(lr[:nG], want_l1rr, (n, "level-1 r.r"))
    same([po.reduce_final(lz[:nG]), po.reduce_final(lr[:nG])], [want_rz, want_rr], (n, "totals"))
    same(dA.get(), Ap, (n, "Ap untouched"))
    same(dd.get(), dinv, (n, "dinv untouched"))
    for v in (dr, dA, dd, dz, dlz, dlr):
        v.free()


def test_update_r_native_without_specials_gives_finite_dots(gpu):
    """the same kernel on clean data: the totals are the tree dots of the updated r with z and with itself"""
    n = 5000
    rng = np.random.default_rng(3)
    r, Ap, dinv = rng.standard_normal(n), rng.standard_normal(n), 1.0 + rng.random(n)
    want_r, want_z, l1rz, l1rr, rz, rr = ref.update_r(r, Ap, dinv, 0.25)
    assert rz == po.ddot_tree(want_r, want_z) and rr == po.ddot_tree(want_r, want_r) and np.isfinite([rz, rr]).all()
    nG = (n + 255) // 256
    dr, dA, dd, dz = DeviceVector.from_host(r), DeviceVector.from_host(Ap), DeviceVector.from_host(dinv), DeviceVector(n)
    dlz, dlr = DeviceVector(nG), DeviceVector(nG)
    gpu.sb_pcg_update_r_native(n, 0.25, dA.ptr, dr.ptr, dd.ptr, dz.ptr, dlz.ptr, dlr.ptr)
    same(dlz.get(), l1rz, "level-1 r.z")
    same(dlr.get(), l1rr, "level-1 r.r")
    for v in (dr, dA, dd, dz, dlz, dlr):
        v.free()
