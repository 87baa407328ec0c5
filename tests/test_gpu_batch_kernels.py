"""The block kernels of batched CG against the single-vector kernels they are twins of, BIT FOR BIT: column c of
sb_spmmv_native == sb_spmv_native on column c, for every format and width, with NaN, +-Inf, -0.0 and subnormals in distinct
columns (a column must not leak into its neighbour); the fused level-1 values of sb_spmmv_native_dot == those of
sb_spmv_native_dot on each column; interleave / de-interleave round trips.  On ragged matrices (empty rows, chunks shorter than
the kernels' unroll, one very long row, nc != nr, chunk counts that leave waves of the last workgroup idle) column c also ==
the oracle's CRS product of column c and, on Sell-64, the level-1 values == the oracle's."""
import os

import numpy as np
import pytest

from conftest import REFDATA
from oracle import pyoracle as po
from sparsebench_amd import hostapi
from sparsebench_amd.capi import DeviceVector
from test_gpu_bicgstab_kernels import same
from test_gpu_kernels import random_csr, upload_crs, upload_scs

pytestmark = pytest.mark.gpu
BAND = os.path.join(REFDATA, "matrix_band_klein.mtx")

SHAPES = {"hpcg8": ("generate", (8, 8, 8)), "hpcg16": ("generate", (16, 16, 16)), "hpcg_10_11_13": ("generate", (10, 11, 13)),
          "band_klein": (BAND, (1, 1, 1)), "irregular12": ("irregular", (12, 12, 12))}
FORMATS = {"crs": ("crs", 64, 1), "sell_64_1": ("scs", 64, 1), "sell_64_256": ("scs", 64, 256), "sell_4_8": ("scs", 4, 8)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def block_input(n, nv, seed):
    """(n, nv) doubles: random, with the special values in distinct columns (kind j lives in column j mod nv only)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, nv))
    tiny = np.float64(5e-324)
    special = [[np.nan], [np.inf, -np.inf], [-0.0], [tiny, -tiny, 1e-310]]
    for j, vals in enumerate(special):
        for t, v in enumerate(vals):
            for row in {(7 * j + 3 * t + 1) % n, (n // 2 + 5 * j + t) % n, (n - 1 - j - 4 * t) % n}:
                X[row, j % nv] = v
    return np.ascontiguousarray(X)


@pytest.mark.parametrize("nv", [2, 4, 8])
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_spmmv_column_equals_spmv_bit_for_bit(gpu, shape, fmt, nv):
    L = gpu
    filename, dims = SHAPES[shape]
    f, Cc, sigma = FORMATS[fmt]
    p = hostapi.Problem(filename, *dims, fmt=f, Cc=Cc, sigma=sigma)
    nr, nc = p.nr, p.nc
    assert nc == nr
    X = block_input(nc, nv, seed=nr + nv)
    dX, dY = DeviceVector.from_host(X.reshape(-1)), DeviceVector.from_host(np.full(nr * nv, 9.9))
    L.sb_spmmv_native(p.matrix, nv, dX.ptr, dY.ptr)
    Y = dY.get().reshape(nr, nv)
    nG = (nr + 255) // 256
    dL = DeviceVector.from_host(np.full(nv * nG + 4, 9.9))
    dY2 = DeviceVector.from_host(np.full(nr * nv, 9.9))
    kind = L.sb_spmmv_native_dot(p.matrix, nv, dX.ptr, dY2.ptr, dL.ptr)
    assert kind == (2 if (f == "scs" and Cc == 64) else 0)
    if kind:
        assert np.array_equal(bits(dY2.get()), bits(Y.reshape(-1)))
        assert np.all(dL.get()[nv * nG:] == 9.9)  # nothing behind the last column's values
    l1 = dL.get()[:nv * nG].reshape(nv, nG)
    dx, dy = DeviceVector(nc), DeviceVector(nr)
    tried = set()
    for mode in (5, 0):  # both single-vector kernels where the matrix has two (the block kernel ignores the mode)
        got = p.use_packed(mode)
        if got in tried:
            continue
        tried.add(got)
        for c in range(nv):
            dx.set(X[:, c].copy())
            dy.set(np.full(nr, 7.7))
            L.sb_spmv_native(p.matrix, dx.ptr, dy.ptr)
            y = dy.get()
            bad = np.nonzero(bits(Y[:, c]) != bits(y))[0]
            assert bad.size == 0, (shape, fmt, nv, mode, c, "first difference at row", int(bad[0]), Y[bad[0], c], y[bad[0]])
            if kind:
                dq = DeviceVector.from_host(np.zeros(4 * nG + 4))
                assert L.sb_spmv_native_dot(p.matrix, dx.ptr, dy.ptr, dq.ptr) == 2
                assert np.array_equal(bits(dq.get()[:nG]), bits(l1[c])), (shape, fmt, nv, mode, c)
                dq.free()
    # the special values stayed in their columns: a column without NaN / Inf in its input has none in its output
    for c in range(nv):
        if np.isfinite(X[:, c]).all():
            assert np.isfinite(Y[:, c]).all(), (shape, fmt, nv, c)
    for d in (dX, dY, dY2, dL, dx, dy):
        d.free()
    p.free()


RAGGED = {"1x1": (1, 1, 1, None), "65x90": (65, 90, 7, None), "1000x1300": (1000, 1300, 40, None), "long_row": (300, 300, 9, 9000),
          "257x64": (257, 64, 64, None), "chunk_lengths_0_to_7": None}
RAGGED_FORMATS = [("crs", 0, 0), ("scs", 64, 1), ("scs", 64, 128), ("scs", 16, 32)]


def ragged_matrix(shape):
    rng = np.random.default_rng(len(shape) + 11)
    if RAGGED[shape] is not None:
        nr, nc, maxlen, long_row = RAGGED[shape]
        return random_csr(rng, nr, nc, maxlen, long_row=long_row)
    # eight blocks of 64 rows, every row of block k with k entries: the Sell-64-1 chunks are 0, 1, .. 7 long -- under, at and past
    # the unroll of 4 (2 at nv = 8) with every remainder
    lens = np.repeat(np.arange(8), 64)
    rp = np.zeros(len(lens) + 1, dtype=np.uint32)
    rp[1:] = np.cumsum(lens)
    g = po.GMatrix.from_csr(rp, rng.integers(0, 600, size=int(rp[-1])).astype(np.uint32), rng.standard_normal(int(rp[-1])), nc=600)
    assert np.array_equal(np.asarray(g.to_scs(64, 1).chunkLens), np.arange(8))
    return g


@pytest.mark.parametrize("nv", [2, 4, 8])
@pytest.mark.parametrize("shape", list(RAGGED))
def test_spmmv_ragged_random_and_long_rows(gpu, shape, nv):
    """the block twin of test_spmv_ragged_random_and_long_rows: spmmv_crs_rows, spmmv_scs64 (with and without its fused dot)
    and spmmv_scs_rows against the oracle's CRS product, column by column"""
    L = gpu
    g = ragged_matrix(shape)
    nr, nc = g.nr, g.nc
    X = block_input(nc, nv, seed=nr + nc + nv)
    assert nr == 1 or np.isfinite(X[0]).all()  # the padding's column: 0.0 * x[0] must stay a zero (one row: no padding is stored)
    want = [g.spmv(np.ascontiguousarray(X[:, c])) for c in range(nv)]
    nG = (nr + 255) // 256
    for f, Cc, sigma in RAGGED_FORMATS:
        what = (shape, nv, f, Cc, sigma)
        sc = g.to_scs(Cc, sigma) if f == "scs" else None
        m = upload_scs(L, sc) if sc else upload_crs(L, g)
        # the device's row order: rows below nr permuted for sigma > 1, the columns behind them as they are; rows that no
        # column index names hold NaN
        rows = max(nr, nc)
        Xd = np.full((rows, nv), np.nan)
        Xd[:nc] = X
        n2o = None
        if L.sb_matrix_is_permuted(m):
            n2o = np.asarray(sc.newToOldPerm).astype(np.int64)
            Xd[:nr] = Xd[:rows][n2o].copy()
        dX, dY = DeviceVector.from_host(Xd.reshape(-1)), DeviceVector.from_host(np.full(nr * nv + 4, 9.9))
        L.sb_spmmv_native(m, nv, dX.ptr, dY.ptr)
        got = dY.get()
        assert np.all(got[nr * nv:] == 9.9), (what, "written behind Y")
        Y = got[:nr * nv].reshape(nr, nv)
        dx, dy = DeviceVector(rows), DeviceVector(nr)
        for c in range(nv):
            same(Y[:, c], want[c][n2o] if n2o is not None else want[c], (what, c, "the oracle's product"))
            dx.set(np.ascontiguousarray(Xd[:, c]))
            dy.set(np.full(nr, 7.7))
            L.sb_spmv_native(m, dx.ptr, dy.ptr)
            same(Y[:, c], dy.get(), (what, c, "sb_spmv_native"))
            if np.isfinite(X[:, c]).all():
                assert np.isfinite(Y[:, c]).all(), (what, c, "a neighbour's special values came over")
        dL, dY2 = DeviceVector.from_host(np.full(nv * nG + 4, 9.9)), DeviceVector.from_host(np.full(nr * nv + 4, 9.9))
        kind = L.sb_spmmv_native_dot(m, nv, dX.ptr, dY2.ptr, dL.ptr)
        assert kind == (2 if (f == "scs" and Cc == 64) else 0)
        if kind and nc >= nr:
            assert np.array_equal(bits(dY2.get()), bits(got)), (what, "Y of the kernel with the fused dot")
            l1 = dL.get()
            assert np.all(l1[nv * nG:] == 9.9), (what, "written behind the last level-1 value")
            for c in range(nv):
                same(l1[c * nG:(c + 1) * nG], po.ddot_partials(np.ascontiguousarray(Xd[:nr, c]), np.ascontiguousarray(Y[:, c])),
                     (what, c, "level-1 values"))
        for d in (dX, dY, dx, dy, dL, dY2):
            d.free()
        L.sb_matrix_free(m)


def test_spmmv_bytes_model(gpu):
    p = hostapi.Problem("generate", 16, 16, 16, fmt="scs", Cc=64, sigma=1)
    one = gpu.sb_matrix_spmv_bytes(p.matrix)
    vec = 8.0 * p.nrPadded + 8.0 * p.nc
    for nv in (2, 4, 8):
        assert gpu.sb_matrix_spmmv_bytes(p.matrix, nv) == (one - vec) + nv * vec
    p.free()


def identity(L, n):
    rp = np.arange(n + 1, dtype=np.uint32)
    col = np.arange(n, dtype=np.uint32)
    val = np.ones(n)
    return L.sb_crs_upload(n, n, rp.ctypes.data_as(hostapi.vp), col.ctypes.data_as(hostapi.vp), val.ctypes.data_as(hostapi.vp))


@pytest.mark.parametrize("nv", [2, 4, 8])
def test_interleave_round_trips(gpu, nv):
    L = gpu
    for n in (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 4097, 100003):
        m = identity(L, n)
        cols = np.arange(n * nv, dtype=np.float64).reshape(nv, n) + 0.25
        dC, dX, dB = DeviceVector.from_host(cols.reshape(-1)), DeviceVector.from_host(np.full(n * nv, -1.0)), DeviceVector(n * nv)
        L.sb_block_interleave(m, nv, dC.ptr, dX.ptr)
        assert np.array_equal(dX.get().reshape(n, nv), cols.T), (n, nv)
        L.sb_block_deinterleave(m, nv, dX.ptr, dB.ptr)
        assert np.array_equal(dB.get(), cols.reshape(-1)), (n, nv)
        for d in (dC, dX, dB):
            d.free()
        L.sb_matrix_free(m)


@pytest.mark.parametrize("nv", [2, 4, 8])
def test_interleave_permutes_for_sigma_above_one(gpu, nv):
    L = gpu
    p = hostapi.Problem("generate", 10, 11, 13, fmt="scs", Cc=64, sigma=256)
    assert L.sb_matrix_is_permuted(p.matrix)
    n = p.nr
    n2o = p.array("newToOldPerm").astype(np.int64)
    assert not np.array_equal(n2o, np.arange(n))
    cols = np.random.default_rng(5).standard_normal((nv, n))
    dC, dX, dB = DeviceVector.from_host(cols.reshape(-1)), DeviceVector(n * nv), DeviceVector(n * nv)
    L.sb_block_interleave(p.matrix, nv, dC.ptr, dX.ptr)
    X = dX.get().reshape(n, nv)
    dv, dp = DeviceVector(n), DeviceVector(n)
    for c in range(nv):
        assert np.array_equal(X[:, c], cols[c][n2o])
        dv.set(cols[c].copy())
        L.sb_permute(p.matrix, dv.ptr, dp.ptr)  # the single-vector path's own permutation
        assert np.array_equal(X[:, c], dp.get())
    L.sb_block_deinterleave(p.matrix, nv, dX.ptr, dB.ptr)
    assert np.array_equal(dB.get(), cols.reshape(-1))
    for d in (dC, dX, dB, dv, dp):
        d.free()
    p.free()
