"""Single-precision kernels on the MI355X, each result bit for bit against tests/sp_ref.py: SpMV (CRS, Sell-64 with sigma 1 and
256, generic C), waxpby, every level of the tree dot and the seq dot; and fp64 calls on an SP matrix are refused."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import sp_ref
from sparsebench_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p
F = np.float32


@pytest.fixture(scope="module")
def L():
    return capi.init(0)


def hp(a):
    return a.ctypes.data_as(vp)


def dev(a, dtype=F):
    return capi.DeviceVector.from_host(np.ascontiguousarray(a, dtype), dtype)


def same_bits(a, b):
    """bit for bit; NaN counts as NaN whatever its sign or payload (x86 and the GPU make different default NaNs)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def ragged(nr, nc, seed, long_row=0, specials=False):
    """CRS with ragged rows (0 .. 40 entries, one of `long_row`), subnormal values and, with specials, NaN / Inf"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 41, nr)
    if long_row:
        lens[nr // 2] = long_row
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    col = rng.integers(0, nc, int(rp[-1])).astype(np.uint32)
    val = rng.standard_normal(int(rp[-1])).astype(F)
    val[::7] *= F(1e-39)  # subnormal values
    val[::11] *= F(1e-20)  # products with x[...] ~ 1e-20 below the normal range
    if specials:
        val[5] = np.inf
        val[17] = np.nan
        val[40] = -np.inf
    x = rng.standard_normal(nc).astype(F)
    x[::13] *= F(1e-20)
    x[::29] = F(1e-42)
    return rp, col, val, x


def scs_layout(rp, col, val, C_, sigma):
    """the reference's Sell-C-sigma layout: rows sorted by descending length inside sigma windows (stable),
    chunk width = longest row, column-major, padding column 0 / value 0"""
    nr = len(rp) - 1
    lens = np.diff(rp).astype(np.int64)
    nCh = (nr + C_ - 1) // C_
    npad = nCh * C_
    plen = np.zeros(npad, np.int64)
    plen[:nr] = lens
    order = np.arange(npad)
    for w in range(0, npad, sigma):
        seg = np.arange(w, min(w + sigma, npad))
        order[w:w + len(seg)] = seg[np.argsort(-plen[seg], kind="stable")]
    widths = plen[order].reshape(nCh, C_).max(axis=1)
    cptr = np.concatenate([[0], np.cumsum(widths * C_)]).astype(np.uint32)
    ne = int(cptr[-1])
    scol, sval = np.zeros(ne, np.uint32), np.zeros(ne, F)
    o2n = np.zeros(nr, np.uint32)
    for q, i in enumerate(order):
        if i >= nr:
            continue
        o2n[i] = q
        at = int(cptr[q // C_]) + q % C_ + C_ * np.arange(lens[i])
        scol[at], sval[at] = col[rp[i]:rp[i + 1]], val[rp[i]:rp[i + 1]]
    n2o = np.zeros(nr, np.uint32)
    n2o[o2n] = np.arange(nr, dtype=np.uint32)
    return nCh, cptr, widths.astype(np.uint32), scol, sval, o2n, n2o


def upload_scs(L, nr, nc, C_, sigma, lay):
    nCh, cptr, cl, scol, sval, o2n, n2o = lay
    return L.sb_scs_upload_f32(nr, nc, C_, sigma, nCh, len(scol), hp(cptr), hp(cl), hp(scol), hp(sval), hp(o2n), hp(n2o))


def run_spmv(L, m, nr, x):
    dx, dy = dev(x), capi.DeviceVector(nr, dtype=F)
    L.sb_spmv_f32(m, dx.ptr, dy.ptr)
    y = dy.get()
    dx.free(), dy.free()
    return y


@pytest.mark.parametrize("long_row,specials", [(0, False), (0, True), (1500, False)])
def test_spmv_crs_f32(L, long_row, specials):
    nr = nc = 3000
    rp, col, val, x = ragged(nr, nc, 1, long_row, specials)
    m = L.sb_crs_upload_f32(nr, nc, hp(rp), hp(col), hp(val))
    assert L.sb_matrix_precision(m) == 1
    assert L.sb_matrix_crs_kernel(m) == (0 if long_row else 1)  # rows > 1025: the row-block kernel
    with np.errstate(all="ignore"):
        ref = sp_ref.spmv_crs(rp, col, val, x)
    assert same_bits(run_spmv(L, m, nr, x), ref)
    L.sb_matrix_free(m)


@pytest.mark.parametrize("C_,sigma,specials", [(64, 1, False), (64, 256, False), (64, 256, True), (8, 1, False), (32, 64, True)])
def test_spmv_scs_f32(L, C_, sigma, specials):
    nr = nc = 2500
    rp, col, val, x = ragged(nr, nc, 2, 0, specials)
    lay = scs_layout(rp, col, val, C_, sigma)
    m = upload_scs(L, nr, nc, C_, sigma, lay)
    with np.errstate(all="ignore"):
        ref = sp_ref.spmv_scs(lay[1], lay[2], lay[3], lay[4], C_, lay[5], nr, x)
        crs = sp_ref.spmv_crs(rp, col, val, x)
    y = run_spmv(L, m, nr, x)
    assert same_bits(y, ref)
    if not specials:
        assert same_bits(y, crs)  # SCS == CRS (padding adds +-0)
    assert L.sb_matrix_spmv_bytes(m) == 8.0 * len(lay[3]) + 8.0 * lay[0] + 4.0 * lay[0] * C_ + 4.0 * nc
    L.sb_matrix_free(m)


def test_spmv_scs64_fused_level1(L):
    """the Sell-64 kernel's fused x . y: one level-1 value per 256 rows = ((q0 + q1) + q2) + q3 of the level-0 butterflies"""
    nr = nc = 5000
    rp, col, val, x = ragged(nr, nc, 3)
    lay = scs_layout(rp, col, val, 64, 1)
    m = upload_scs(L, nr, nc, 64, 1, lay)
    dx, dy = dev(x), capi.DeviceVector(nr, dtype=F)
    q = capi.DeviceVector((nr + 255) // 256, np.zeros((nr + 255) // 256), F)
    assert L.sb_spmv_native_dot_f32(m, dx.ptr, dy.ptr, q.ptr) == 2
    y = dy.get()
    assert same_bits(y, sp_ref.spmv_crs(rp, col, val, x))
    assert same_bits(q.get(), sp_ref.level1(sp_ref.level0(x[:nr], y)))
    L.sb_matrix_free(m)


@pytest.mark.parametrize("alpha,beta", [(1.0, 0.37), (-0.71, 1.0), (2.5, -1.25), (1.0, 0.0), (1.0, 1.0)])
@pytest.mark.parametrize("alias", ["none", "x", "y"])
def test_waxpby_f32(L, alpha, beta, alias):
    rng = np.random.default_rng(4)
    n = 10007
    x, y = rng.standard_normal(n).astype(F), rng.standard_normal(n).astype(F)
    x[::9] *= F(1e-40)
    y[::5] = F(-0.0)
    dx, dy = dev(x), dev(y)
    dw = dx if alias == "x" else dy if alias == "y" else capi.DeviceVector(n, dtype=F)
    L.sb_waxpby_f32(n, alpha, dx.ptr, beta, dy.ptr, dw.ptr)
    assert same_bits(dw.get(), sp_ref.waxpby(alpha, x, beta, y))


@pytest.mark.parametrize("n", [1, 63, 257, 5000, 300001])
def test_dot_levels_f32(L, n):
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n).astype(F), rng.standard_normal(n).astype(F)
    a[::17] *= F(1e-25)
    da, db = dev(a), dev(b)
    m = (n + 255) // 256
    q = capi.DeviceVector(4 * m, dtype=F)
    L.sb_ddot_partials_f32(n, da.ptr, db.ptr, q.ptr)
    l0 = q.get()
    assert same_bits(l0, sp_ref.level0(a, b))
    out = capi.DeviceVector(1, dtype=F)
    L.sb_reduce_final_f32(m, q.ptr, out.ptr)
    assert same_bits(out.get()[0], sp_ref.level2(sp_ref.level1(l0)))
    old = L.sb_dot_order()
    try:
        L.sb_set_dot_order(0)
        assert same_bits(L.sb_ddot_f32(n, da.ptr, db.ptr), sp_ref.dot_tree(a, b))
        L.sb_set_dot_order(1)
        assert same_bits(L.sb_ddot_f32(n, da.ptr, db.ptr), sp_ref.dot_seq(a, b))
        assert same_bits(L.sb_ddot_f32(n, da.ptr, da.ptr), sp_ref.dot_seq(a, a))
    finally:
        L.sb_set_dot_order(old)


CROSS = {
    "spmv_fp64_on_sp": "L.sb_spmv(m, d, d)",
    "cg_create_fp64_on_sp": "L.sb_cg_create(m, None, hp(np.ones(p.nr)), None)",
    "use_packed_on_sp": "L.sb_matrix_use_packed(m, 5)",
    "cg_create_f32_on_dp": "L.sb_cg_create_f32(q.matrix, None, hp(np.ones(q.nr, np.float32)), None)",
}


@pytest.mark.parametrize("case", sorted(CROSS))
def test_crossing_precisions_is_fatal(case):
    """in a child process: the call ends it with EXIT_FAILURE and a file:line message"""
    code = "\n".join([
        "import sys, numpy as np, ctypes as C",
        "sys.path.insert(0, %r)" % ROOT,
        "from sparsebench_amd import capi, hostapi",
        "L = capi.init(0)",
        "hp = lambda a: a.ctypes.data_as(C.c_void_p)",
        "p = hostapi.Problem('generate', 8, 8, 8, fmt='scs', precision='single')",
        "q = hostapi.Problem('generate', 8, 8, 8, fmt='crs')",
        "m = p.matrix",
        "d = L.sb_malloc(8 * p.nc)",
        "L.sb_matrix_use_packed(m, 0)",  # (mode 0 is allowed)
        CROSS[case],
        "L.sb_sync()",
        "print('NOT REFUSED')",
    ])
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "NOT REFUSED" not in r.stdout
    assert "precision" in r.stderr and ".h:" in r.stderr, r.stderr[-2000:]
