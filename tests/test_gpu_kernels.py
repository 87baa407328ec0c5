"""Parity of the HIP kernels against the oracle, through the C-ABI (ctypes), on the
same inputs.  Bar: BIT-EXACT for SpMV (per-row order kept), waxpby (elementwise) and
both stages of the fixed-order dot."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import REFDATA, load_json, modes_scs
from oracle import pyoracle as po
from sparsebench_amd import capi, hostapi
from sparsebench_amd.capi import DeviceVector

pytestmark = pytest.mark.gpu
vp = C.c_void_p


def _p(a):
    return a.ctypes.data_as(vp)


def upload_crs(L, g):
    rp, col, val = (np.ascontiguousarray(a) for a in (g.rowPtr, g.col, g.val))
    return L.sb_crs_upload(g.nr, g.nc, _p(rp), _p(col), _p(val))


def upload_scs(L, s):
    arrs = [np.ascontiguousarray(a) for a in (s.chunkPtr, s.chunkLens, s.colInd, s.val,
                                              s.oldToNewPerm, s.newToOldPerm)]
    return L.sb_scs_upload(s.nr, s.nc, s.C, s.sigma, s.nChunks, s.nElems, *[_p(a) for a in arrs])


def gpu_spmv(L, m, x, nr):
    """y = A x through the C-ABI; when the matrix has a compressed mirror, BOTH kernels
    (packed stream and reference-layout stream) must give the same bits"""
    dx, dy = DeviceVector.from_host(x), DeviceVector(nr)
    L.sb_spmv(m, dx.ptr, dy.ptr)
    y = dy.get()
    # every kernel the matrix has (0 reference stream / native CRS, 5 masked row programs; CRS: through its private
    # mirror) must give the same bits.
    # Where the result is NaN only the NaN-ness is compared (which NaN payload an add of two NaNs returns depends
    # on operand order, not on the algorithm)
    best = L.sb_matrix_packed_mode(m)
    tried = set()
    for mode in (0, 5):
        L.sb_matrix_use_packed(m, mode)
        got = L.sb_matrix_packed_mode(m)
        if got in tried:
            continue
        tried.add(got)
        dy.set(np.full(nr, 7.0))
        L.sb_spmv(m, dx.ptr, dy.ptr)
        y2 = dy.get()
        nan = np.isnan(y)
        assert np.array_equal(nan, np.isnan(y2)), "kernel mode %d: NaN rows differ" % got
        assert np.array_equal(y[~nan].view(np.uint64), y2[~nan].view(np.uint64)), "kernel mode %d differs" % got
    assert best in tried
    L.sb_matrix_use_packed(m, best)
    dx.free(), dy.free()
    return y


def random_csr(rng, nr, nc, maxlen, empty_rows=True, long_row=None):
    lens = rng.integers(0 if empty_rows else 1, maxlen + 1, size=nr)
    if long_row is not None:
        lens[rng.integers(0, nr)] = long_row
    rp = np.zeros(nr + 1, dtype=np.uint32)
    rp[1:] = np.cumsum(lens)
    col = rng.integers(0, nc, size=int(rp[-1])).astype(np.uint32)
    val = rng.standard_normal(int(rp[-1]))
    return po.GMatrix.from_csr(rp, col, val, nc=nc)


MATS = ["test%d" % i for i in range(11)] + ["matrix_band_klein"]


@pytest.mark.parametrize("name", MATS)
def test_spmv_reference_matrices_all_formats(gpu, name):
    L = gpu
    g = po.GMatrix.from_mtx(os.path.join(REFDATA, name + ".mtx"))
    ref = np.array([float(v) for v in load_json("spmv_ref.json")[name]])
    x = np.ones(g.nc)
    m = upload_crs(L, g)
    assert np.array_equal(gpu_spmv(L, m, x, g.nr), ref)
    L.sb_matrix_free(m)
    rng = np.random.default_rng(1)
    xr = rng.standard_normal(g.nc)
    for Cc, sg in ((1, 1), (2, 1), (4, 1), (4, 8), (64, 1), (64, 16), (128, 4), (3, 5)):
        s = g.to_scs(Cc, sg)
        m = upload_scs(L, s)
        assert np.array_equal(gpu_spmv(L, m, x, g.nr), ref), (Cc, sg)
        assert np.array_equal(gpu_spmv(L, m, xr, g.nr), g.spmv(xr)), (Cc, sg)
        L.sb_matrix_free(m)


@pytest.mark.parametrize("n", [4, 8, 17, 32])
def test_spmv_hpcg_bit_exact(gpu, n):
    L = gpu
    g = po.GMatrix.generate(n, n + 1, n + 2)
    rng = np.random.default_rng(n)
    x = rng.standard_normal(g.nc)
    y = g.spmv(x)
    m = upload_crs(L, g)
    assert np.array_equal(gpu_spmv(L, m, x, g.nr), y)
    L.sb_matrix_free(m)
    for Cc, sg in ((64, 1), (64, 256), (64, 1000000), (32, 64), (256, 512)):
        s = g.to_scs(Cc, sg)
        m = upload_scs(L, s)
        assert L.sb_matrix_is_permuted(m) == int(not np.array_equal(s.oldToNewPerm, np.arange(s.nr)))
        assert np.array_equal(gpu_spmv(L, m, x, g.nr), y), (Cc, sg)
        # native (permuted-space) call agrees with the oracle's literal chunk order
        xp = x[np.asarray(s.newToOldPerm)] if L.sb_matrix_is_permuted(m) else x
        dx, dy = DeviceVector.from_host(xp), DeviceVector(g.nr)
        L.sb_spmv_native(m, dx.ptr, dy.ptr)
        assert np.array_equal(dy.get(), s.spmv_literal(x)[:g.nr]), (Cc, sg)
        dx.free(), dy.free()
        L.sb_matrix_free(m)


def test_spmv_ragged_random_and_long_rows(gpu):
    """empty rows, rows longer than one LDS tile (CRS), ragged chunks, nc > nr"""
    L = gpu
    rng = np.random.default_rng(11)
    for nr, nc, maxlen, long_row in ((1, 1, 1, None), (65, 90, 7, None), (1000, 1300, 40, None),
                                     (300, 300, 9, 9000), (5000, 5000, 3, 4097), (257, 64, 64, None)):
        g = random_csr(rng, nr, nc, maxlen, long_row=long_row)
        x = rng.standard_normal(nc)
        y = g.spmv(x)
        m = upload_crs(L, g)
        assert np.array_equal(gpu_spmv(L, m, x, nr), y), ("crs", nr, long_row)
        L.sb_matrix_free(m)
        for Cc, sg in ((64, 1), (64, 128), (16, 32)):
            s = g.to_scs(Cc, sg)
            m = upload_scs(L, s)
            assert np.array_equal(gpu_spmv(L, m, x, nr), y), ("scs", nr, Cc, sg)
            L.sb_matrix_free(m)


def test_crs_equal_nonzero_windows_edge_cases(gpu):
    """spmv_crs_split (tiles = equal windows of nonzeros; kernels.hip.h): more than 256 rows in a tile (short and empty rows:
    threads loop), no nonzeros at all, empty rows behind the last nonzero, rows that end exactly on / start exactly at a window
    boundary, the longest row the kernel takes (1025: T = 1024) and the first length it leaves to the row-block kernel"""
    L = gpu
    rng = np.random.default_rng(77)

    def check(lens, nc, want_split):
        lens = np.asarray(lens, dtype=np.int64)
        rp = np.zeros(len(lens) + 1, dtype=np.uint32)
        rp[1:] = np.cumsum(lens)
        col = rng.integers(0, nc, size=int(rp[-1])).astype(np.uint32)
        val = rng.standard_normal(int(rp[-1]))
        g = po.GMatrix.from_csr(rp, col, val, nc=nc)
        x = rng.standard_normal(nc)
        m = upload_crs(L, g)
        assert L.sb_matrix_crs_kernel(m) == (1 if want_split else 0), (len(lens), int(lens.max(initial=0)))
        assert np.array_equal(gpu_spmv(L, m, x, g.nr), g.spmv(x)), (len(lens), int(lens.max(initial=0)))
        L.sb_matrix_free(m)

    check(rng.integers(0, 4, size=20000), 500, True)            # ~1400 rows per tile
    check(np.zeros(3000), 10, True)                              # no nonzeros: one tile, 3000 empty rows
    check(np.r_[rng.integers(1, 30, size=4000), np.zeros(700)], 4000, True)   # empty rows behind the last nonzero
    check(np.r_[np.zeros(300), rng.integers(1, 30, size=4000)], 4000, True)   # ... and in front of the first
    check(np.full(4096, 31), 4096, True)                         # T = 1984 = 64 rows of 31: rows end exactly on the boundaries
    check(np.r_[np.full(64, 31), [0, 0, 0], np.full(640, 31)], 999, True)     # empty rows exactly at a boundary
    check(np.r_[rng.integers(0, 9, size=900), [1025], rng.integers(0, 9, size=900)], 2000, True)
    check(np.r_[rng.integers(0, 9, size=900), [1026], rng.integers(0, 9, size=900)], 2000, False)
    check(np.full(9, 1025), 1500, True)                          # every row the longest


def test_packed_stream_levels_and_wide_chunks(gpu):
    """the lossless compressed mirror: dictionary on/off, 16-bit and 32-bit (wide) chunks,
    padding marker, sigma > 1 (renumbered padding column), chunk widths 0..9 mod 4"""
    L = gpu
    rng = np.random.default_rng(23)
    # (a) few distinct values + banded columns -> level 2, narrow
    g = po.GMatrix.generate(9, 8, 7)
    for sg in (1, 64, 4096):
        s = g.to_scs(64, sg)
        m = upload_scs(L, s)
        assert L.sb_matrix_pack_level(m) == 2
        x = rng.standard_normal(g.nc)
        assert np.array_equal(gpu_spmv(L, m, x, g.nr), g.spmv(x))
        if L.sb_matrix_packed_mode(m) == 5:  # (the mirror is streamed only through its row programs)
            assert L.sb_matrix_stream_bytes(m) < 0.45 * L.sb_matrix_spmv_bytes(m)
        else:
            assert L.sb_matrix_packed_mode(m) == 0 and L.sb_matrix_stream_bytes(m) == L.sb_matrix_spmv_bytes(m)
        L.sb_matrix_free(m)
    # (b) random values (no dictionary) + columns spread over a huge range -> level 1, wide chunks
    for nr, nc, maxlen in ((700, 300000, 11), (129, 70000, 5), (64, 65535, 3), (64, 65536 + 64, 4)):
        gm = random_csr(rng, nr, nc, maxlen)
        x = rng.standard_normal(nc)
        for sg in (1, 128):
            s = gm.to_scs(64, sg)
            m = upload_scs(L, s)
            distinct = len(np.unique(np.concatenate([gm.val, [0.0]]).view(np.uint64)))
            assert L.sb_matrix_pack_level(m) == (2 if distinct <= 256 else 1)
            assert np.array_equal(gpu_spmv(L, m, x, nr), gm.spmv(x)), (nr, nc, sg)
            L.sb_matrix_free(m)
    # (c) exactly 256 / 257 distinct values: dictionary boundary; explicit zeros and -0.0 kept
    for nvals, level in ((255, 2), (256, 1)):  # +0.0 for padding is always in the dictionary
        nr = 400
        rp = np.arange(0, 3 * nr + 1, 3, dtype=np.uint32)
        col = rng.integers(0, nr, size=3 * nr).astype(np.uint32)
        pool = np.concatenate([np.arange(1, nvals - 1, dtype=np.float64) * 0.37, [-0.0, np.inf]])[:nvals]
        val = pool[np.arange(3 * nr) % nvals]
        gm = po.GMatrix.from_csr(rp, col, val, nc=nr)
        s = gm.to_scs(64, 1)
        m = upload_scs(L, s)
        assert L.sb_matrix_pack_level(m) == level, (nvals, L.sb_matrix_pack_level(m))
        x = rng.standard_normal(nr)
        got, exp = gpu_spmv(L, m, x, nr), gm.spmv(x)
        assert np.array_equal(got.view(np.uint64), exp.view(np.uint64))
        L.sb_matrix_free(m)


def test_masked_row_programs_the_products_compressed_kernel(gpu):
    """what ships next to the reference-layout stream: the masked row programs (level 6, mode 5).  Built for every chunk
    of stencils with lines of >= 128 rows (with and without the sigma sort), the default wherever built, any other mode
    request falls to 5 or 0, bit-identical to the oracle incl. NaN / Inf reaching exactly the rows the reference lets
    them reach (Sell-C-sigma padding multiplies x[padCol])."""
    L = gpu
    rng = np.random.default_rng(29)
    for dims, sg, full in (((128, 128, 2), 256, True), ((128, 128, 2), 1, True), ((16, 16, 16), 1, False), ((70, 3, 5), 1, False),
                           ((20, 5, 33), 4096, False), ((9, 8, 7), 64, False)):
        g = po.GMatrix.generate(*dims)
        s = g.to_scs(64, sg)
        m = upload_scs(L, s)
        mch = C.c_uint32(0)
        progs = L.sb_matrix_row_programs(m, C.byref(mch))
        if full:
            assert progs >= 1 and mch.value == s.nChunks, (dims, sg, progs, mch.value)
        assert L.sb_matrix_packed_mode(m) == (5 if progs else 0)
        for want in (1, 2, 3, 4, 5, 7):
            L.sb_matrix_use_packed(m, want)
            assert L.sb_matrix_packed_mode(m) == (5 if progs and want >= 5 else 0), (dims, sg, want)
        L.sb_matrix_use_packed(m, 5)
        x = rng.standard_normal(g.nc)
        assert np.array_equal(gpu_spmv(L, m, x, g.nr), g.spmv(x))
        x[0], x[g.nc // 2] = np.inf, np.nan
        got, exp = gpu_spmv(L, m, x, g.nr), s.spmv(x)
        assert np.isnan(exp).any() and np.array_equal(np.isnan(got), np.isnan(exp))
        ok = ~np.isnan(exp)
        assert np.array_equal(got[ok].view(np.uint64), exp[ok].view(np.uint64))
        L.sb_matrix_free(m)


def test_spmv_empty_matrix(gpu):
    L = gpu
    g = po.GMatrix.from_csr(np.zeros(4, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(0), nc=3)
    m = upload_crs(L, g)
    assert np.array_equal(gpu_spmv(L, m, np.ones(3), 3), np.zeros(3))
    L.sb_matrix_free(m)
    s = g.to_scs(64, 1)
    m = upload_scs(L, s)
    assert np.array_equal(gpu_spmv(L, m, np.ones(3), 3), np.zeros(3))
    L.sb_matrix_free(m)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 4097, 100003, 1 << 20])
def test_waxpby_and_ddot_bit_exact(gpu, n):
    L = gpu
    rng = np.random.default_rng(n + 5)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    dx, dy, dw = DeviceVector.from_host(x), DeviceVector.from_host(y), DeviceVector(n)
    for a, b in ((1.0, -0.37), (2.5, 1.0), (2.5, -3.0), (1.0, 0.0), (0.0, 0.0)):
        L.sb_waxpby(n, a, dx.ptr, b, dy.ptr, dw.ptr)
        assert np.array_equal(dw.get(), po.waxpby(a, x, b, y)), (a, b)
    # aliasing as solveCG uses it: w == y (src/CGSolver.c:114) and w == x (:127)
    L.sb_waxpby(n, 1.0, dx.ptr, 0.5, dy.ptr, dy.ptr)
    y2 = po.waxpby(1.0, x, 0.5, y)
    assert np.array_equal(dy.get(), y2)
    L.sb_waxpby(n, 1.0, dx.ptr, -2.0, dy.ptr, dx.ptr)
    x2 = po.waxpby(1.0, x, -2.0, y2)
    assert np.array_equal(dx.get(), x2)
    # fixed-order dot, both stages
    m = (n + 255) // 256
    dq = DeviceVector.from_host(np.full(max(4 * m, 1), 9.9))  # level 0: 4 partials per 256 elements
    L.sb_ddot_partials(n, dx.ptr, dy.ptr, dq.ptr)
    if m:
        q = dq.get()[:4 * m].reshape(m, 4)
        assert np.all(q.reshape(-1)[(n + 63) // 64:] == 0.0)  # tail zeroed
        lvl1 = ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]      # level 1, same IEEE adds
        assert np.array_equal(lvl1, po.ddot_partials(x2, y2))
        dres = DeviceVector(1)
        L.sb_reduce_final(m, dq.ptr, dres.ptr)
        assert dres.get()[0] == po.ddot_tree(x2, y2)
        dres.free()
    assert L.sb_ddot(n, dx.ptr, dy.ptr) == po.ddot_tree(x2, y2)
    assert L.sb_ddot(n, dx.ptr, dx.ptr) == po.ddot_tree(x2, x2)
    if n:
        seq = po.ddot_seq(x2, y2)
        bound = (n - 1) * 2.0 ** -53 * float(np.sum(np.abs(x2 * y2))) + 1e-300
        assert abs(L.sb_ddot(n, dx.ptr, dy.ptr) - seq) <= bound
    for v in (dx, dy, dw, dq):
        v.free()


def test_fused_dot_partials_of_the_spmv(gpu):
    """the p . Ap partials the CG loop takes out of the SpMV launch: per 64 rows (device order) the butterfly of x_i * y_i,
    combined per aligned 256 rows ((q0 + q1) + q2) + q3 by the kernel itself -- equal to the oracle's level-1 partials of
    the same two vectors, for every kernel mode with a fused dot"""
    L = gpu
    rng = np.random.default_rng(41)
    for dims, sg in (((128, 128, 2), 256), ((32, 32, 32), 1), ((70, 3, 5), 1), ((20, 5, 33), 64)):
        g = po.GMatrix.generate(*dims)
        s = g.to_scs(64, sg)
        m = upload_scs(L, s)
        x = rng.standard_normal(g.nc)
        xp = x[np.asarray(s.newToOldPerm)] if L.sb_matrix_is_permuted(m) else x  # the device's (permuted) order
        dx, dy = DeviceVector.from_host(xp), DeviceVector(s.nr)
        nq = 4 * ((s.nr + 255) // 256)
        tried = set()
        for mode in modes_scs():
            L.sb_matrix_use_packed(m, mode)
            got = L.sb_matrix_packed_mode(m)
            if got in tried:
                continue
            tried.add(got)
            dq = DeviceVector.from_host(np.zeros(nq))
            kind = L.sb_spmv_native_dot(m, dx.ptr, dy.ptr, dq.ptr)
            assert got in (0, 5) and kind == 2  # both kernels emit level-1 values
            y, lvl1 = dy.get(), dq.get()[:nq // 4]
            assert not dq.get()[nq // 4:].any()  # nothing behind the last 256-group
            assert np.array_equal(lvl1.view(np.uint64), po.ddot_partials(xp[:s.nr].copy(), y).view(np.uint64)), (dims, sg, got)
            dq.free()
        assert len(tried) >= (2 if dims[0] >= 128 else 1)
        dx.free(), dy.free()
        L.sb_matrix_free(m)


def test_ddot_run_to_run_reproducible(gpu):
    L = gpu
    rng = np.random.default_rng(2)
    x = rng.standard_normal(3_000_017)
    dx = DeviceVector.from_host(x)
    vals = {L.sb_ddot(len(x), dx.ptr, dx.ptr) for _ in range(5)}
    assert len(vals) == 1 and vals.pop() == po.ddot_tree(x, x)
    dx.free()


def test_special_values_propagate_like_the_cpu(gpu):
    """-0.0, inf and NaN take the same path through mul/add as on the CPU"""
    L = gpu
    x = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan, 1e308, -1e308, 5e-324] * 9)
    y = np.array([1.0, -0.0, 0.0, 2.0, 1.0, 10.0, 10.0, 0.5] * 9)
    dx, dy, dw = DeviceVector.from_host(x), DeviceVector.from_host(y), DeviceVector(len(x))
    L.sb_waxpby(len(x), 1.0, dx.ptr, 0.0, dy.ptr, dw.ptr)
    got, exp = dw.get(), po.waxpby(1.0, x, 0.0, y)
    assert np.array_equal(got.view(np.uint64), exp.view(np.uint64))
    for v in (dx, dy, dw):
        v.free()


def test_pattern_levels_randomised_shapes(gpu, monkeypatch):
    """levels 4-5 on matrices that are regular enough to qualify but ragged everywhere else: random
    subsets of a small offset set (many odd rows: mixed U and L chunks, exception staging), rows wider
    than 32 columns (streamed code groups / pattern entries past the prefetch), duplicate columns, empty
    rows, several far-apart offsets (> 6 window segments: the slot-by-slot staging and the segment
    overflow list), sigma on and off.  Every kernel mode must give the oracle's bits."""
    L = gpu
    monkeypatch.setenv("SB_PACK_LDS", "1")  # the window heuristic would refuse most of these
    rng = np.random.default_rng(31)
    built = 0
    for trial in range(10):
        nr = int(rng.integers(300, 2600))
        far = trial % 3 == 0
        offs = np.array([-1500, -700, -260, 0, 300, 900, 1400] if far else [-70, -9, -2, -1, 0, 1, 2, 11])
        vals = np.array([4.0, -1.0, -0.25])
        common = rng.random(nr) < (0.85 if trial % 2 == 0 else 0.4)
        rows, cols, data = [0], [], []
        for i in range(nr):
            if rng.random() < 0.02:
                pick = np.array([], dtype=np.int64)  # empty row
            elif common[i]:
                pick = offs
            elif trial >= 5 and rng.random() < 0.1:
                pick = rng.choice(offs, size=int(rng.integers(33, 45)))  # wide row, duplicate columns
            else:
                pick = np.sort(rng.choice(offs, size=int(rng.integers(1, len(offs) + 1)), replace=False))
            pick = pick[(i + pick >= 0) & (i + pick < nr)]  # offsets that leave the matrix are dropped
            c = i + pick
            cols.append(c)
            data.append(np.where(pick == 0, vals[0], np.where(np.abs(pick) < 5, vals[1], vals[2])))
            rows.append(rows[-1] + len(c))
        rp = np.array(rows, dtype=np.uint32)
        col = np.concatenate(cols).astype(np.uint32)
        val = np.concatenate(data).astype(np.float64)
        gm = po.GMatrix.from_csr(rp, col, val, nc=nr)
        x = rng.standard_normal(nr)
        for sg in (1, 256):
            s = gm.to_scs(64, sg)
            m = upload_scs(L, s)
            built += L.sb_matrix_pattern_classes(m) > 0
            got, exp = gpu_spmv(L, m, x, nr), gm.spmv(x)
            assert np.array_equal(got.view(np.uint64), exp.view(np.uint64)), (trial, sg, L.sb_matrix_packed_mode(m))
            L.sb_matrix_free(m)
    assert built >= 12, built  # most of the 20 really reach the pattern levels


def test_crs_through_its_pattern_mirror(gpu, monkeypatch):
    """CRS matrices with repeating row patterns get a device-private Sell-64-1 mirror whose padding is
    NOT added (src/matrix-CRS.c:46-65 has no padding): same bits as the oracle's CRS loop, also where
    the Sell-C-sigma semantics would differ (Inf / NaN in x[0], which SCS padding multiplies by 0)"""
    L = gpu
    rng = np.random.default_rng(37)
    for dims in ((16, 16, 16), (128, 128, 2), (70, 3, 5), (9, 8, 7)):
        g = po.GMatrix.generate(*dims)
        m = upload_crs(L, g)
        # (a mirror is kept only where it carries row programs)
        assert L.sb_matrix_pattern_classes(m) >= 1 or not L.sb_matrix_row_programs(m, None), dims
        if dims[0] >= 128:
            assert L.sb_matrix_row_programs(m, None) >= 1
        # default: through the mirror's masked row programs where it has them, else (small matrix) the native kernel
        assert L.sb_matrix_packed_mode(m) == (5 if L.sb_matrix_row_programs(m, None) else 0)
        x = rng.standard_normal(g.nc)
        assert np.array_equal(gpu_spmv(L, m, x, g.nr).view(np.uint64), g.spmv(x).view(np.uint64))
        x[0], x[g.nc // 2] = np.inf, np.nan
        L.sb_matrix_use_packed(m, 3)
        got, exp = gpu_spmv(L, m, x, g.nr), g.spmv(x)
        assert np.isnan(exp).any() and not np.isnan(exp).all()
        assert np.array_equal(np.isnan(got), np.isnan(exp))  # only the rows that really touch x[0] / the NaN
        ok = ~np.isnan(exp)
        assert np.array_equal(got[ok].view(np.uint64), exp[ok].view(np.uint64))
        L.sb_matrix_free(m)
    # ragged rows, an empty row, duplicate columns, -0.0 and explicit zeros away from column 0
    nr = 700
    offs = np.array([-9, -2, -1, 0, 1, 2, 11])
    rows, cols, data = [0], [], []
    for i in range(nr):
        pick = offs if rng.random() < 0.8 else np.sort(rng.choice(offs, size=int(rng.integers(0, 7)), replace=False))
        pick = pick[(i + pick >= 1) & (i + pick < nr)]  # column 0 stays unused
        cols.append(i + pick)
        data.append(np.where(pick == 0, 4.0, np.where(pick == 11, 0.0, np.where(pick == -9, -0.0, -1.0))))
        rows.append(rows[-1] + len(pick))
    gm = po.GMatrix.from_csr(np.array(rows, dtype=np.uint32), np.concatenate(cols).astype(np.uint32),
                             np.concatenate(data), nc=nr)
    monkeypatch.setenv("SB_PACK_LDS", "1")
    m = upload_crs(L, gm)
    x = rng.standard_normal(nr)
    x[5] = np.inf
    got, exp = gpu_spmv(L, m, x, nr), gm.spmv(x)
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    assert np.array_equal(got[ok].view(np.uint64), exp[ok].view(np.uint64))
    L.sb_matrix_free(m)
    # a stored +0.0 at column 0 cannot be told from padding: no mirror, native kernel only
    col0 = gm.col.copy()
    val0 = gm.val.copy()
    col0[3], val0[3] = 0, 0.0
    gz = po.GMatrix.from_csr(np.array(rows, dtype=np.uint32), col0, val0, nc=nr)
    m = upload_crs(L, gz)
    assert L.sb_matrix_pattern_classes(m) == 0 and L.sb_matrix_packed_mode(m) == 0
    got, exp = gpu_spmv(L, m, x, nr), gz.spmv(x)
    ok = ~np.isnan(exp)
    assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.array_equal(got[ok].view(np.uint64), exp[ok].view(np.uint64))
    L.sb_matrix_free(m)


def test_placement_tuner_picks_memory_by_measurement_and_changes_no_bit(gpu, monkeypatch):
    """Round 4: which device memory the reference-layout stream sits in decides how fast spmv_scs64 reads it (the same
    arrays in a series of fresh allocations of one process: 128 / 128 / 114 / 115 ... us per launch), so the upload copies the
    stream into a few fresh slabs, times the kernel on each and keeps the fastest; sb_cg_create does the same for the loop's
    vectors.  Same bytes, same kernel: the product and the CG history are the bits of the untuned run."""
    n = 96  # 884 736 rows: a 282 MB stream (tuned)
    rng = np.random.default_rng(11)
    outs = {}
    for place in ("0", "1"):
        monkeypatch.setenv("SB_PLACE", place)
        prob = hostapi.Problem("generate", n, n, n, fmt="scs", Cc=64, sigma=256)
        assert prob.use_packed(0) == 0
        rep = prob.placement_report()
        if place == "0":
            assert rep is None
        else:
            assert rep["probes_timed"] >= 3 and rep["us_kept"] <= rep["us_first_pair"] <= rep["us_slowest"] * 1.0001
        x = rng.standard_normal(prob.nc) if not outs else outs["x"]
        outs["x"] = x
        dx, dy = DeviceVector.from_host(x), DeviceVector(prob.nr)
        gpu.sb_spmv_native(prob.matrix, dx.ptr, dy.ptr)
        cg = hostapi.CG(prob)
        cg.solve(12, 0.0)
        outs[place] = (dy.get().copy(), cg.history())
        dx.free(), dy.free(), cg.free(), prob.free()
    assert np.array_equal(outs["0"][0], outs["1"][0])
    assert np.array_equal(outs["0"][1][0], outs["1"][1][0]) and np.array_equal(outs["0"][1][1], outs["1"][1][1])


def test_placement_tuner_gives_back_everything_it_held(gpu, monkeypatch):
    """the search of DESIGN 4.1 holds fresh allocations (arenas, spacers, slabs, one of them managed memory) until it ends; what it
    does not keep it frees, and freeing the matrix frees the rest: the device's free memory after three upload / solve / free
    cycles is what it was after the first (which pays for one-time pools of the runtime)."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    free_b, total_b = C.c_size_t(0), C.c_size_t(0)

    def free_now():
        gpu.sb_sync()
        assert hip.hipMemGetInfo(C.byref(free_b), C.byref(total_b)) == 0
        return free_b.value

    monkeypatch.setenv("SB_PLACE", "1")
    seen = []
    for _ in range(3):
        prob = hostapi.Problem("generate", 96, 96, 96, fmt="scs", Cc=64, sigma=256)
        assert prob.placement_report()["probes_timed"] >= 1
        held = free_now()
        cg = hostapi.CG(prob)
        cg.solve(5, 0.0)
        cg.free(), prob.free()
        seen.append((held, free_now()))
    # while the matrix lives: the stream, the mirror and the kept arena -- well under 1 GiB at 96^3, not the search's gigabytes
    assert seen[1][1] - seen[1][0] < (1 << 30) and seen[2][1] - seen[2][0] < (1 << 30)
    assert abs(seen[2][1] - seen[0][1]) <= (64 << 20), seen  # nothing accumulates from cycle to cycle
