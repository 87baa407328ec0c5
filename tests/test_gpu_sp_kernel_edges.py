"""The single-precision kernels on the MI355X at their edges, each result bit for bit against tests/sp_ref.py (the sizes and
matrices of the fp64 tests in tests/test_gpu_kernels.py, in float): waxpby from n = 0 to 2^20 in its three branches, every
level of the tree dot on the 64 / 256 / 1024 / 262 144 boundaries, the seq dot around its 16-wide chain and its 8192-element
blocks, CRS rows longer than the LDS tile and the equal-window edge cases, Sell-C-sigma with fewer than 64 rows, halo columns
(nc > nr), a chunk of width 0 and no nonzeros at all."""
import numpy as np
import pytest

import sp_ref
from sparsebench_amd import capi
from test_gpu_sp_kernels import L, dev, hp, run_spmv, same_bits, scs_layout, upload_scs  # noqa: F401  (L: the fixture)

pytestmark = pytest.mark.gpu
F = np.float32


# ---- waxpby -------------------------------------------------------------------------------------------------------------------
def waxpby_inputs(n):
    rng = np.random.default_rng(n + 4)
    x, y = rng.standard_normal(n).astype(F), rng.standard_normal(n).astype(F)
    x[::9] *= F(1e-40)  # subnormal
    y[::5] = F(-0.0)
    return x, y


BRANCHES = [(1.0, 0.37), (-0.71, 1.0), (2.5, -1.25)]  # alpha == 1 | beta == 1 | neither (src/solver.c:16-39)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, 100003, 1 << 20])
def test_waxpby_f32_sizes(L, n):
    x, y = waxpby_inputs(n)
    dx, dy, dw = dev(x), dev(y), capi.DeviceVector(n, np.full(n, 7.0), F)
    for alpha, beta in BRANCHES + [(1.0, 1.0), (1.0, 0.0)]:
        L.sb_waxpby_f32(n, alpha, dx.ptr, beta, dy.ptr, dw.ptr)
        assert same_bits(dw.get(), sp_ref.waxpby(alpha, x, beta, y)), (alpha, beta)
    dx.free(), dy.free(), dw.free()


@pytest.mark.parametrize("n", [1, 257, 100003])
@pytest.mark.parametrize("alias", ["none", "x", "y"])
def test_waxpby_f32_aliased(L, n, alias):
    """w == y is src/CGSolver.c:114, w == x is :127"""
    x, y = waxpby_inputs(n)
    for alpha, beta in BRANCHES:
        dx, dy = dev(x), dev(y)
        dw = dx if alias == "x" else dy if alias == "y" else capi.DeviceVector(n, dtype=F)
        L.sb_waxpby_f32(n, alpha, dx.ptr, beta, dy.ptr, dw.ptr)
        assert same_bits(dw.get(), sp_ref.waxpby(alpha, x, beta, y)), (alpha, beta)
        if alias != "x":
            assert same_bits(dx.get(), x)
        if alias != "y":
            assert same_bits(dy.get(), y)
        dx.free(), dy.free()
        if alias == "none":
            dw.free()


# ---- the tree dot -------------------------------------------------------------------------------------------------------------
def with_dot_order(L, order, fn):
    old = L.sb_dot_order()
    try:
        L.sb_set_dot_order(order)
        return fn()
    finally:
        L.sb_set_dot_order(old)


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 262143, 262144, 262145, 262144 + 256 + 1])
def test_tree_dot_levels_f32(L, n):
    """level 0 (4 per 256 elements, +0.0 behind n), levels 1-2 of sb_reduce_final_f32 (the last four sizes: 1024, 1024, 1025 and
    1026 level-1 values, so a second trip over the 1024 threads for one or two of them) and the whole sb_ddot_f32"""
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n).astype(F), rng.standard_normal(n).astype(F)
    a[::17] *= F(1e-25)
    da, db = dev(a), dev(b)
    m = (n + 255) // 256
    q = capi.DeviceVector(4 * m, np.full(4 * m, 9.5), F)
    L.sb_ddot_partials_f32(n, da.ptr, db.ptr, q.ptr)
    l0 = q.get()
    assert same_bits(l0, sp_ref.level0(a, b))
    assert not l0[(n + 63) // 64:].view(np.uint32).any()  # +0.0 behind the last 64-group
    out = capi.DeviceVector(1, dtype=F)
    L.sb_reduce_final_f32(m, q.ptr, out.ptr)
    l1 = sp_ref.level1(sp_ref.level0(a, b))
    assert len(l1) == m
    assert same_bits(out.get()[0], sp_ref.level2(l1))
    assert same_bits(with_dot_order(L, 0, lambda: L.sb_ddot_f32(n, da.ptr, db.ptr)), sp_ref.dot_tree(a, b))
    assert same_bits(with_dot_order(L, 0, lambda: L.sb_ddot_f32(n, da.ptr, da.ptr)), sp_ref.dot_tree(a, a))
    da.free(), db.free(), q.free(), out.free()


# ---- the seq dot --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32, 33, 8191, 8192, 8193, 8192 + 15, 16384, 16385])
def test_seq_dot_f32(L, n):
    """the 16-wide pipelined chain (cnt < 16: the scalar tail alone; 16, 32: no tail) and its two LDS blocks of 8192 (exactly one,
    one more element, exactly two, two and one)"""
    rng = np.random.default_rng(n + 1)
    a, b = rng.standard_normal(n).astype(F), rng.standard_normal(n).astype(F)
    a[::17] *= F(1e-25)
    da, db = dev(a), dev(b)
    assert same_bits(with_dot_order(L, 1, lambda: L.sb_ddot_f32(n, da.ptr, db.ptr)), sp_ref.dot_seq(a, b))
    assert same_bits(with_dot_order(L, 1, lambda: L.sb_ddot_f32(n, da.ptr, da.ptr)), sp_ref.dot_seq(a, a))
    da.free(), db.free()


def test_seq_dot_f32_through_subnormals(L):
    """every product and every partial sum of the chain is subnormal or cancels back through the subnormal range"""
    n = 8192 + 15
    rng = np.random.default_rng(5)
    a = (rng.standard_normal(n) * 1e-20).astype(F)
    b = (rng.standard_normal(n) * 1e-20).astype(F)
    prods = a * b
    ref = sp_ref.dot_seq(a, b)
    tiny = np.finfo(F).tiny
    assert np.sum((prods != 0) & (np.abs(prods) < tiny)) > n // 2 and ref != 0 and abs(ref) < tiny
    da, db = dev(a), dev(b)
    assert same_bits(with_dot_order(L, 1, lambda: L.sb_ddot_f32(n, da.ptr, db.ptr)), ref)
    assert same_bits(with_dot_order(L, 0, lambda: L.sb_ddot_f32(n, da.ptr, db.ptr)), sp_ref.dot_tree(a, b))
    da.free(), db.free()


# ---- CRS ----------------------------------------------------------------------------------------------------------------------
def crs_of(lens, nc, rng):
    """CRS with the given row lengths: random columns, values with subnormals and products below the normal range"""
    lens = np.asarray(lens, np.int64)
    rp = np.zeros(len(lens) + 1, np.uint32)
    rp[1:] = np.cumsum(lens)
    nnz = int(rp[-1])
    col = rng.integers(0, nc, nnz).astype(np.uint32)
    val = rng.standard_normal(nnz).astype(F)
    val[::7] *= F(1e-39)
    val[::11] *= F(1e-20)
    x = rng.standard_normal(nc).astype(F)
    x[::13] *= F(1e-20)
    return rp, col, val, x


def check_crs(L, lens, nc, rng, want_split):
    rp, col, val, x = crs_of(lens, nc, rng)
    nr = len(rp) - 1
    m = L.sb_crs_upload_f32(nr, nc, hp(rp), hp(col), hp(val))
    what = (nr, nc, int(np.max(lens, initial=0)))
    assert L.sb_matrix_crs_kernel(m) == (1 if want_split else 0), what
    assert same_bits(run_spmv(L, m, nr, x), sp_ref.spmv_crs(rp, col, val, x)), what
    L.sb_matrix_free(m)
    return rp, col, val, x


@pytest.mark.parametrize("long_row", [2048, 2049, 4097, 9000])
def test_crs_rows_longer_than_the_tile(L, long_row):
    """spmv_crs_stream_f32: a row of exactly one tile (2048), and rows walked tile by tile -- a second tile of one product, a
    third of one product, five tiles"""
    rng = np.random.default_rng(long_row)
    lens = rng.integers(0, 10, 300)
    lens[150] = long_row
    check_crs(L, lens, 300, rng, False)
    lens = rng.integers(0, 4, 70)  # ... as the first and as the last row
    lens[0], lens[-1] = long_row, long_row + 1
    check_crs(L, lens, 5000, rng, False)


def test_crs_equal_nonzero_windows_edge_cases_f32(L):
    """spmv_crs_split_f32: the cases of test_crs_equal_nonzero_windows_edge_cases (tests/test_gpu_kernels.py) in float"""
    rng = np.random.default_rng(77)
    check_crs(L, rng.integers(0, 4, size=20000), 500, rng, True)             # ~1400 rows per tile: threads loop
    check_crs(L, np.zeros(3000), 10, rng, True)                              # no nonzeros: one tile, 3000 empty rows
    check_crs(L, np.r_[rng.integers(1, 30, size=4000), np.zeros(700)], 4000, rng, True)  # empty rows behind the last nonzero
    check_crs(L, np.r_[np.zeros(300), rng.integers(1, 30, size=4000)], 4000, rng, True)  # ... and in front of the first
    check_crs(L, np.full(4096, 31), 4096, rng, True)                         # T = 1984 = 64 rows of 31: rows end on the boundaries
    check_crs(L, np.r_[np.full(64, 31), [0, 0, 0], np.full(640, 31)], 999, rng, True)    # empty rows exactly at a boundary
    check_crs(L, np.r_[rng.integers(0, 9, size=900), [1025], rng.integers(0, 9, size=900)], 2000, rng, True)
    check_crs(L, np.r_[rng.integers(0, 9, size=900), [1026], rng.integers(0, 9, size=900)], 2000, rng, False)
    check_crs(L, np.full(9, 1025), 1500, rng, True)                          # every row the longest


LAYOUTS = [(64, 1), (64, 128), (16, 32)]


def check_scs(L, rp, col, val, x, nc, C_, sigma):
    nr = len(rp) - 1
    lay = scs_layout(rp, col, val, C_, sigma)
    m = upload_scs(L, nr, nc, C_, sigma, lay)
    y = run_spmv(L, m, nr, x)
    assert same_bits(y, sp_ref.spmv_scs(lay[1], lay[2], lay[3], lay[4], C_, lay[5], nr, x)), (nr, nc, C_, sigma)
    assert same_bits(y, sp_ref.spmv_crs(rp, col, val, x)), (nr, nc, C_, sigma)  # finite inputs: the padding adds +-0
    L.sb_matrix_free(m)
    return lay


@pytest.mark.parametrize("nr,nc,maxlen", [(1, 1, 1), (65, 90, 7), (257, 64, 64)])
def test_spmv_small_and_rectangular_f32(L, nr, nc, maxlen):
    """one row; nc > nr (halo columns: sb_spmv_f32 carries them behind the permuted part); nc < nr with rows up to 64 entries"""
    rng = np.random.default_rng(11 + nr)
    lens = rng.integers(0, maxlen + 1, nr)
    if nr == 1:
        lens[0] = 1
    rp, col, val, x = check_crs(L, lens, nc, rng, True)
    if nc > nr:
        assert (col >= nr).any()
    permuted = 0
    for C_, sigma in LAYOUTS:
        lay = check_scs(L, rp, col, val, x, nc, C_, sigma)
        permuted += int(not np.array_equal(lay[5], np.arange(nr)))
    if nr > 1:
        assert permuted  # the halo copy of sb_spmv_f32 runs for permuted matrices only


@pytest.mark.parametrize("nr", [1, 63, 64, 65])
@pytest.mark.parametrize("C_,sigma", LAYOUTS)
def test_spmv_scs_f32_around_one_chunk(L, nr, C_, sigma):
    """fewer rows than a chunk, exactly one, one more; nc > nr"""
    nc = nr + 25
    rng = np.random.default_rng(100 * nr + C_)
    lens = rng.integers(0, 12, nr)
    lens[rng.integers(0, nr)] = 17
    rp, col, val, x = crs_of(lens, nc, rng)
    assert (col >= nr).any()
    check_scs(L, rp, col, val, x, nc, C_, sigma)


def native_dot(L, m, lay, rp, col, val, nr, nc, seed):
    """sb_spmv_native_dot_f32 in the device's row order: y and one level-1 value of x . y per 256 rows"""
    o2n, n2o = lay[5].astype(np.int64), lay[6].astype(np.int64)
    xd = np.random.default_rng(seed).standard_normal(nc).astype(F)  # in the device's order
    xd[::17] *= F(1e-25)
    xo = xd.copy()
    xo[:nr] = xd[o2n]
    ref = sp_ref.spmv_crs(rp, col, val, xo)[n2o]
    nq = (nr + 255) // 256
    dx, dy, q = dev(xd), capi.DeviceVector(nr, np.full(nr, 7.0), F), capi.DeviceVector(nq, np.full(nq, 7.0), F)
    assert L.sb_spmv_native_dot_f32(m, dx.ptr, dy.ptr, q.ptr) == 2
    y = dy.get()
    assert same_bits(y, ref)
    assert same_bits(q.get(), sp_ref.level1(sp_ref.level0(xd[:nr], y)))
    dx.free(), dy.free(), q.free()


@pytest.mark.parametrize("nr", [65, 5001])
@pytest.mark.parametrize("sigma", [1, 128])
def test_fused_level1_with_idle_waves_in_the_last_block(L, nr, sigma):
    """nr = 65: two chunks, so two of the block's four waves hold no chunk; nr = 5001: 79 chunks, the last block has one idle
    wave -- spmv_scs64_f32<DOT> still writes that block's level-1 value, with +0.0 for the rows that are not there"""
    nc = nr
    rng = np.random.default_rng(nr + sigma)
    rp, col, val, _ = crs_of(rng.integers(0, 30, nr), nc, rng)
    lay = scs_layout(rp, col, val, 64, sigma)
    assert lay[0] % 4 in (2, 3)
    m = upload_scs(L, nr, nc, 64, sigma, lay)
    native_dot(L, m, lay, rp, col, val, nr, nc, 3)
    L.sb_matrix_free(m)


def test_scs_chunks_of_width_zero_f32(L):
    """the last 64 rows are empty: at sigma = 1 the last chunk has width 0 (and one in the middle too); y = +0.0 there"""
    nr = nc = 320
    rng = np.random.default_rng(8)
    lens = rng.integers(1, 20, nr)
    lens[128:192] = 0
    lens[256:] = 0
    rp, col, val, x = crs_of(lens, nc, rng)
    lay = scs_layout(rp, col, val, 64, 1)
    assert list(lay[2] == 0) == [False, False, True, False, True]
    for C_, sigma in LAYOUTS:
        check_scs(L, rp, col, val, x, nc, C_, sigma)
    m = upload_scs(L, nr, nc, 64, 1, lay)
    y = run_spmv(L, m, nr, x)
    assert not y[256:].view(np.uint32).any() and not y[128:192].view(np.uint32).any()
    native_dot(L, m, lay, rp, col, val, nr, nc, 4)
    L.sb_matrix_free(m)


@pytest.mark.parametrize("nr,nc", [(3, 3), (130, 7), (300, 300)])
def test_no_nonzeros_at_all_f32(L, nr, nc):
    rng = np.random.default_rng(nr)
    rp, col, val, x = check_crs(L, np.zeros(nr), nc, rng, True)
    assert len(col) == 0
    for C_, sigma in LAYOUTS:
        lay = check_scs(L, rp, col, val, x, nc, C_, sigma)
        assert len(lay[3]) == 0
    if nc == nr:
        lay = scs_layout(rp, col, val, 64, 1)
        m = upload_scs(L, nr, nc, 64, 1, lay)
        y = run_spmv(L, m, nr, x)
        assert not y.view(np.uint32).any()  # +0.0, not -0.0
        native_dot(L, m, lay, rp, col, val, nr, nc, 6)
        L.sb_matrix_free(m)
