"""The opt-in single-precision mirror on the MI355X (sb_set_sp_mirror / SB_SP_MIRROR; csrc/pack_sp.hip.h): where it is built
(exactly where the fp64 upload turns every chunk into a row program), and that spmv_prog_f32 and the 3-launch loop over
spmv_prog_fusep_f32 give the bits of tests/sp_ref.py, of the streaming kernels and of the reference's own SP history.
Everything is bit for bit; NaN results compare by NaN-ness."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sp_ref
from sparsebench_amd import capi, hostapi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BAND = os.path.join(GOLDEN, "ref", "matrix_band_klein.mtx")
BIN = os.path.join(ROOT, "sparsebench_amd", "bin")
vp = C.c_void_p
F = np.float32


@pytest.fixture(scope="module")
def L():
    return capi.init(0)


@pytest.fixture(autouse=True)
def no_placement_tuner(monkeypatch):
    """the fp64 twins are uploaded for their structure only: skip the placement tuner's timing runs"""
    monkeypatch.setenv("SB_PLACE", "0")


def hp(a):
    return a.ctypes.data_as(vp)


def dev(a, dtype=F):
    return capi.DeviceVector.from_host(np.ascontiguousarray(a, dtype), dtype)


def bits(a):
    a = np.asarray(a, F)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def same_bits(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def problem(shape, fmt, sigma, precision="single", mirror=None):
    if shape == "band_klein":
        return hostapi.Problem(BAND, 1, 1, 1, fmt=fmt, Cc=64, sigma=sigma, precision=precision, mirror=mirror)
    nx, ny, nz = shape
    return hostapi.Problem("generate", nx, ny, nz, fmt=fmt, Cc=64, sigma=sigma, precision=precision, mirror=mirror)


def fp64_all_row_programs(shape, fmt, sigma):
    q = problem(shape, fmt, sigma, precision="double")
    a = q.all_row_programs()
    q.free()
    return a


# ---- 1. where it is built -----------------------------------------------------------------------------------------------------
# The small shapes that carry most of the tests: (128,128,2) as Sell-64-1, Sell-64-256 and CRS.  sb_matrix_all_row_programs of
# their fp64 uploads is 1 on the MI355X (test_the_mirror_is_built_where_fp64_has_all_row_programs asserts it every run).
SMALL = [((128, 128, 2), "scs", 1), ((128, 128, 2), "scs", 256), ((128, 128, 2), "crs", 1)]
MUST = [((128, 128, 128), "scs", 256), ((256, 256, 256), "scs", 256)]
# Shapes where fp64 may or may not have all row programs: the SP mirror must follow it either way.  (On the MI355X: 1 for 16^3
# in every format and for CRS 128^3; 0 for (70,3,5) and matrix_band_klein.mtx, which therefore walk the not-built branch.)
OTHER = [((16, 16, 16), "scs", 1), ((16, 16, 16), "scs", 256), ((16, 16, 16), "crs", 1), ((70, 3, 5), "scs", 1),
         ((70, 3, 5), "crs", 1), ("band_klein", "scs", 1), ("band_klein", "crs", 1), ((128, 128, 128), "crs", 1)]


def check_built(p):
    assert p.all_row_programs() == 1
    assert p.pack_info()["mode"] == 5
    cg = hostapi.CG(p, dot_order="tree")
    assert cg.fuse_p() == 1 and cg.launches_per_body() == 3
    cg.free()
    assert p.stream_bytes() < p.spmv_bytes()
    assert p.use_packed(0) == 0 and p.stream_bytes() == p.spmv_bytes()
    assert p.use_packed(5) == 5


@pytest.mark.parametrize("shape,fmt,sigma", MUST + SMALL)
def test_the_mirror_is_built_where_fp64_has_all_row_programs(L, shape, fmt, sigma):
    """never skipped: HPCG 128^3 and 256^3 as Sell-64-256 (fp64 takes the fused p update on them) and the small shapes"""
    assert fp64_all_row_programs(shape, fmt, sigma) == 1
    p = problem(shape, fmt, sigma, mirror=True)
    check_built(p)
    p.free()


USE5 = "\n".join([
    "import sys",
    "sys.path.insert(0, %r)" % ROOT,
    "from sparsebench_amd import capi, hostapi",
    "L = capi.init(0)",
    "shape, fmt, sigma = eval(sys.argv[1]), sys.argv[2], int(sys.argv[3])",
    "f, n = (%r, (1, 1, 1)) if shape == 'band_klein' else ('generate', shape)" % BAND,
    "p = hostapi.Problem(f, n[0], n[1], n[2], fmt=fmt, Cc=64, sigma=sigma, precision='single', mirror=True)",
    "print('ALL', p.all_row_programs(), flush=True)",
    "L.sb_matrix_use_packed(p.matrix, 5)",
    "L.sb_sync()",
    "print('NOT REFUSED')",
])


def device_free_bytes(L):
    L.sb_sync()
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def spmv_and_cg(L, p, iters=25):
    rng = np.random.default_rng(7)
    x = rng.standard_normal(p.nc).astype(F)
    dx, dy = dev(x), capi.DeviceVector(p.nr, dtype=F)
    L.sb_spmv_f32(p.matrix, dx.ptr, dy.ptr)
    y = dy.get()
    dx.free(), dy.free()
    cg = hostapi.CG(p, dot_order="tree")
    k = cg.solve(iters)
    rr, pap = cg.history()
    xs = cg.solution()
    cg.free()
    return y, k, rr, pap, xs


@pytest.mark.parametrize("shape,fmt,sigma", OTHER + SMALL)
def test_every_shape_is_built_exactly_where_fp64_is(L, shape, fmt, sigma):
    """sb_matrix_all_row_programs(SP with the switch on) == the fp64 upload's; where not built the matrix is an upload with the
    switch off: mode 0, use_packed(5) fatal, the same SpMV and CG bits, the same device memory.  Switch off: nothing is built"""
    want = fp64_all_row_programs(shape, fmt, sigma)
    assert L.sb_sp_mirror() == 0
    off = problem(shape, fmt, sigma)  # the process default
    assert off.all_row_programs() == 0 and off.pack_info()["mode"] == 0 and off.stream_bytes() == off.spmv_bytes()
    off.free()
    before = device_free_bytes(L)
    off = problem(shape, fmt, sigma, mirror=False)
    used_off = before - device_free_bytes(L)
    assert off.all_row_programs() == 0 and off.pack_info()["mode"] == 0 and off.stream_bytes() == off.spmv_bytes()
    ref = spmv_and_cg(L, off)
    off.free()
    before = device_free_bytes(L)
    p = problem(shape, fmt, sigma, mirror=True)
    used_on = before - device_free_bytes(L)
    assert p.all_row_programs() == want
    got = spmv_and_cg(L, p)
    assert got[1] == ref[1]
    for u, v in zip((got[0],) + got[2:], (ref[0],) + ref[2:]):
        assert same_bits(u, v)
    if want:
        check_built(p)
    else:
        assert p.pack_info()["mode"] == 0 and p.stream_bytes() == p.spmv_bytes()
        assert used_on == used_off
        cg = hostapi.CG(p, dot_order="tree")
        assert cg.fuse_p() == 0 and cg.launches_per_body() == (3 if fmt == "scs" else 4)
        cg.free()
        r = subprocess.run([sys.executable, "-c", USE5, repr(shape), fmt, str(sigma)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "ALL 0" in r.stdout and "NOT REFUSED" not in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
        assert "a single-precision matrix streams its reference layout only" in r.stderr and ".h:" in r.stderr, r.stderr[-2000:]
    p.free()


def ragged(nr, nc, seed):
    """CRS with ragged rows (0 .. 40 entries) and a distinct value per entry: no value dictionary, the chain stops at level 1"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 41, nr)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    col = rng.integers(0, nc, int(rp[-1])).astype(np.uint32)
    val = rng.standard_normal(int(rp[-1])).astype(F)
    return rp, col, val, rng.standard_normal(nc).astype(F)


def scs_layout(rp, col, val, C_, sigma):
    """the reference's Sell-C-sigma layout: rows sorted by descending length inside sigma windows (stable), chunk width =
    longest row, column-major, padding column 0 / value 0"""
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


def upload_direct(L, fmt, sigma, rp, col, val, nc, mirror):
    """(matrix, layout) through sb_crs_upload_f32 / sb_scs_upload_f32 with the switch set around the call"""
    nr = len(rp) - 1
    old = L.sb_sp_mirror()
    L.sb_set_sp_mirror(1 if mirror else 0)
    try:
        if fmt == "crs":
            return L.sb_crs_upload_f32(nr, nc, hp(rp), hp(col), hp(val)), None
        lay = scs_layout(rp, col, val, 64, sigma)
        nCh, cptr, cl, scol, sval, o2n, n2o = lay
        return L.sb_scs_upload_f32(nr, nc, 64, sigma, nCh, len(scol), hp(cptr), hp(cl), hp(scol), hp(sval), hp(o2n), hp(n2o)), lay
    finally:
        L.sb_set_sp_mirror(old)


def run_spmv(L, m, nr, x):
    dx, dy = dev(x), capi.DeviceVector(nr, dtype=F)
    L.sb_spmv_f32(m, dx.ptr, dy.ptr)
    y = dy.get()
    dx.free(), dy.free()
    return y


@pytest.mark.parametrize("fmt,sigma", [("crs", 1), ("scs", 1), ("scs", 256)])
def test_a_ragged_matrix_with_many_values_gets_no_mirror(L, fmt, sigma):
    nr = nc = 3000
    rp, col, val, x = ragged(nr, nc, 11)
    assert len(np.unique(val.view(np.uint32))) > 256
    if fmt == "crs":
        d = L.sb_crs_upload(nr, nc, hp(rp), hp(col), hp(val.astype(np.float64)))
    else:
        nCh, cptr, cl, scol, sval, o2n, n2o = scs_layout(rp, col, val, 64, sigma)
        d = L.sb_scs_upload(nr, nc, 64, sigma, nCh, len(scol), hp(cptr), hp(cl), hp(scol), hp(sval.astype(np.float64)), hp(o2n), hp(n2o))
    assert L.sb_matrix_all_row_programs(d) == 0
    L.sb_matrix_free(d)
    before = device_free_bytes(L)
    off, _ = upload_direct(L, fmt, sigma, rp, col, val, nc, False)
    used_off = before - device_free_bytes(L)
    y_off = run_spmv(L, off, nr, x)
    L.sb_matrix_free(off)
    before = device_free_bytes(L)
    m, _ = upload_direct(L, fmt, sigma, rp, col, val, nc, True)
    assert before - device_free_bytes(L) == used_off
    assert L.sb_matrix_all_row_programs(m) == 0 and L.sb_matrix_packed_mode(m) == 0
    assert L.sb_matrix_stream_bytes(m) == L.sb_matrix_spmv_bytes(m)
    y = run_spmv(L, m, nr, x)
    assert same_bits(y, y_off) and same_bits(y, sp_ref.spmv_crs(rp, col, val, x))
    L.sb_matrix_free(m)


RAGGED_CHILD = "\n".join([
    "import sys, ctypes as C, numpy as np",
    "sys.path.insert(0, %r)" % ROOT,
    "from sparsebench_amd import capi",
    "L = capi.init(0)",
    "hp = lambda a: a.ctypes.data_as(C.c_void_p)",
    "rng = np.random.default_rng(11)",
    "nr = nc = 3000",
    "rp = np.concatenate([[0], np.cumsum(rng.integers(0, 41, nr))]).astype(np.uint32)",
    "col = rng.integers(0, nc, int(rp[-1])).astype(np.uint32)",
    "val = rng.standard_normal(int(rp[-1])).astype(np.float32)",
    "assert L.sb_sp_mirror() == 1",  # from the environment
    "m = L.sb_crs_upload_f32(nr, nc, hp(rp), hp(col), hp(val))",
    "print('ALL', L.sb_matrix_all_row_programs(m), 'MODE', L.sb_matrix_packed_mode(m), flush=True)",
    "L.sb_matrix_use_packed(m, 0)",  # (mode 0 is allowed)
    "L.sb_matrix_use_packed(m, 5)",
    "L.sb_sync()",
    "print('NOT REFUSED')",
])


def test_use_packed_5_without_a_mirror_stays_fatal_with_the_switch_on():
    """in a child process with SB_SP_MIRROR=1: the ragged matrix gets no mirror (the report line says so), and mode 5 on it
    ends the process with today's message"""
    env = dict(os.environ, SB_SP_MIRROR="1", SB_SP_MIRROR_REPORT="1")
    r = subprocess.run([sys.executable, "-c", RAGGED_CHILD], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 1, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "ALL 0 MODE 0" in r.stdout and "NOT REFUSED" not in r.stdout
    assert "SP_MIRROR built=0 fmt=crs" in r.stderr and "reason=" in r.stderr, r.stderr[-2000:]
    assert "a single-precision matrix streams its reference layout only" in r.stderr and ".h:" in r.stderr, r.stderr[-2000:]


# ---- 2. SpMV ------------------------------------------------------------------------------------------------------------------
def x_vectors(nc):
    rng = np.random.default_rng(3)
    plain = rng.standard_normal(nc).astype(F)
    odd = plain.copy()
    odd[::13] = F(-0.0)
    odd[5::29] = F(1e-42)  # subnormal
    odd[7::31] *= F(1e-30)
    out = {"random": plain, "zeros_subnormals": odd}
    for name, v in (("inf0", np.inf), ("nan0", np.nan)):
        t = odd.copy()
        t[0] = v
        out[name] = t
    for name, v in (("inf_mid", -np.inf), ("nan_mid", np.nan)):
        t = odd.copy()
        t[nc // 2 + 3] = v
        out[name] = t
    return out


@pytest.mark.parametrize("shape,fmt,sigma", SMALL)
def test_spmv_through_the_mirror(L, shape, fmt, sigma):
    p = problem(shape, fmt, sigma, mirror=True)
    assert p.all_row_programs() == 1 and p.pack_info()["mode"] == 5
    c = problem(shape, "crs", 1)
    rp, col, val = c.array("rowPtr").copy(), c.array("crs_colInd").copy(), c.values().copy()
    for name, x in x_vectors(p.nc).items():
        with np.errstate(all="ignore"):
            if fmt == "scs":  # the padding term carries a non-finite x[0] into the rows the reference's loop carries it into
                ref = sp_ref.spmv_scs(p.array("chunkPtr"), p.array("chunkLens"), p.array("scs_colInd"), p.values(), 64,
                                      p.array("oldToNewPerm"), p.nr, x)
            else:
                ref = sp_ref.spmv_crs(rp, col, val, x)
        assert p.use_packed(5) == 5
        y5 = run_spmv(L, p.matrix, p.nr, x)
        assert p.use_packed(0) == 0
        y0 = run_spmv(L, p.matrix, p.nr, x)
        assert same_bits(y5, ref), name
        assert same_bits(y5, y0), name
        if name in ("random", "zeros_subnormals"):
            assert same_bits(y5, sp_ref.spmv_crs(rp, col, val, x)), name
    c.free(), p.free()


@pytest.mark.parametrize("shape,fmt,sigma", SMALL)
def test_fused_level1_through_the_mirror(L, shape, fmt, sigma):
    """sb_spmv_native_dot_f32 in mode 5: y and the level-1 values of x . y in the device's row order (CRS too: return code 2)"""
    p = problem(shape, fmt, sigma, mirror=True)
    assert p.pack_info()["mode"] == 5
    c = problem(shape, "crs", 1)
    rp, col, val = c.array("rowPtr").copy(), c.array("crs_colInd").copy(), c.values().copy()
    nr = p.nr
    xd = np.random.default_rng(5).standard_normal(p.nc).astype(F)  # in the device's order
    xd[::17] *= F(1e-25)
    if fmt == "scs" and sigma > 1:
        o2n, n2o = p.array("oldToNewPerm").astype(np.int64), p.array("newToOldPerm").astype(np.int64)
        ref = sp_ref.spmv_crs(rp, col, val, xd[o2n])[n2o]
    else:
        ref = sp_ref.spmv_crs(rp, col, val, xd)
    dx, dy = dev(xd), capi.DeviceVector(nr, dtype=F)
    q = capi.DeviceVector((nr + 255) // 256, np.zeros((nr + 255) // 256), F)
    assert L.sb_spmv_native_dot_f32(p.matrix, dx.ptr, dy.ptr, q.ptr) == 2
    y = dy.get()
    assert same_bits(y, ref)
    assert same_bits(q.get(), sp_ref.level1(sp_ref.level0(xd[:nr], y)))
    if fmt == "crs":
        assert p.use_packed(0) == 0
        assert L.sb_spmv_native_dot_f32(p.matrix, dx.ptr, dy.ptr, q.ptr) == 0  # the native CRS kernel has no fused dot
    dx.free(), dy.free(), q.free(), c.free(), p.free()


@pytest.mark.parametrize("fmt,sigma", [("crs", 1), ("scs", 1), ("scs", 256)])
def test_the_bit_embedding_keeps_every_float(L, fmt, sigma):
    """a stencil pattern whose values come from a pool with -0.0f, a subnormal, Inf and two NaNs of different payload (one value
    per column offset, so rows still share programs): the mirror is built and multiplies to sp_ref's bits / NaN-ness"""
    c = problem((128, 128, 2), "crs", 1)
    rp, col = c.array("rowPtr").copy(), c.array("crs_colInd").copy()
    nr, nc = c.nr, c.nc
    c.free()
    rows = np.repeat(np.arange(nr, dtype=np.int64), np.diff(rp.astype(np.int64)))
    d = col.astype(np.int64) - rows
    offs = np.unique(d)
    pool = np.array([-0.0, 1e-40, 1.5, -2.25, 26.0, 3e-39, -1.0, 0.125], F)
    table = pool[np.arange(len(offs)) % len(pool)].copy()
    tb = table.view(np.uint32)
    tb[0], tb[1] = 0x7FC00001, 0xFFA00002  # two NaNs, the second a signalling one with the sign set
    table[-1] = np.inf
    val = table[np.searchsorted(offs, d)]
    assert {0x80000000, 0x7FC00001, 0xFFA00002, 0x7F800000} <= set(np.unique(val.view(np.uint32)).tolist())
    m, lay = upload_direct(L, fmt, sigma, rp, col, val, nc, True)
    assert L.sb_matrix_all_row_programs(m) == 1 and L.sb_matrix_packed_mode(m) == 5
    x = np.random.default_rng(9).standard_normal(nc).astype(F)
    with np.errstate(all="ignore"):
        ref = sp_ref.spmv_crs(rp, col, val, x) if fmt == "crs" else sp_ref.spmv_scs(lay[1], lay[2], lay[3], lay[4], 64, lay[5], nr, x)
    assert 0 < np.isnan(ref).sum() < nr and np.isinf(ref).any() and np.isfinite(ref).any()
    y5 = run_spmv(L, m, nr, x)
    L.sb_matrix_use_packed(m, 0)
    y0 = run_spmv(L, m, nr, x)
    assert same_bits(y5, ref) and same_bits(y0, ref)
    L.sb_matrix_free(m)


# ---- 3. CG, tree order ----------------------------------------------------------------------------------------------------------
def solve(p, itermax, eps=0.0, order="tree", **kw):
    cg = hostapi.CG(p, dot_order=order, **kw)
    info = (cg.fuse_p(), cg.launches_per_body())
    k = cg.solve(itermax, eps)
    rr, pap = cg.history()
    x = cg.solution()
    cg.free()
    return (k, rr, pap, x), info


def equal_runs(a, b):
    return a[0] == b[0] and all(same_bits(u, v) for u, v in zip(a[1:], b[1:]))


@pytest.mark.parametrize("shape,fmt,sigma", SMALL)
def test_cg_through_the_mirror(L, shape, fmt, sigma):
    iters = 40
    p = problem(shape, fmt, sigma, mirror=True)
    assert p.pack_info()["mode"] == 5
    a, info = solve(p, iters)
    assert info == (1, 3)
    b, info = solve(p, iters, fuse_p=0)
    assert info == (0, 3)  # the mirror kernel forms level 1 itself, for CRS too
    c, info = solve(p, iters, fused=False)
    assert info == (0, 0)
    assert p.use_packed(0) == 0
    d, info = solve(p, iters)
    assert info == (0, 3 if fmt == "scs" else 4)
    assert a[0] == iters and len(a[1]) == iters - 1
    assert equal_runs(a, b) and equal_runs(a, c) and equal_runs(a, d)
    if sigma == 1:  # the tree runs over the device's row order: the original one
        q = problem(shape, "crs", 1)
        rp, col, val = q.array("rowPtr").copy(), q.array("crs_colInd").copy(), q.values().copy()
        bvec, _ = q.rhs()
        ref = sp_ref.cg(lambda v: sp_ref.spmv_crs(rp, col, val, v), bvec, iters)
        assert equal_runs(a, ref)
        q.free()
    # itermax 0 .. 3 and an exit through eps, against the streaming loop
    eps = float((np.sqrt(np.float64(a[1][9])) + np.sqrt(np.float64(a[1][10]))) / 2)
    for mode in (0, 5):
        assert p.use_packed(mode) == mode
        runs = [solve(p, im)[0] for im in range(4)] + [solve(p, iters, eps)[0]]
        if mode == 0:
            want = runs
    assert all(equal_runs(u, v) for u, v in zip(runs, want))
    assert runs[4][0] < iters and runs[4][0] == len(runs[4][1]) + 1
    # pieces == one solve; finish after 1, 2, 3, 8 bodies takes the owed x update from the right p buffer
    for pieces in ([3, 4, 1, 7, 40], [1], [2], [3], [8]):
        got = {}
        for mode in (0, 5):
            assert p.use_packed(mode) == mode
            cg = hostapi.CG(p, dot_order="tree")
            assert cg.fuse_p() == (1 if mode == 5 else 0)
            cg.start(iters, 0.0)
            for n in pieces:
                cg.run_iters(n)
            k = cg.finish()
            rr, pap = cg.history()
            got[mode] = (k, rr, pap, cg.solution())
            cg.free()
        assert equal_runs(got[5], got[0]), pieces
        if sum(pieces) >= iters:
            assert equal_runs(got[5], a)
        else:
            assert len(got[5][2]) == sum(pieces)  # that many bodies ran
    p.free()


@pytest.mark.parametrize("shape,fmt,sigma", SMALL)
@pytest.mark.parametrize("first,second", [(0, 5), (5, 0)])
def test_a_mode_change_between_pieces_keeps_the_latched_plan(L, shape, fmt, sigma, first, second):
    iters = 14
    p = problem(shape, fmt, sigma, mirror=True)
    assert p.use_packed(first) == first
    ref, (plan, _) = solve(p, iters)
    assert plan == (1 if first == 5 else 0)
    cg = hostapi.CG(p, dot_order="tree")
    cg.start(iters, 0.0)
    cg.run_iters(3)
    assert p.use_packed(second) == second  # mid-solve: the kernel mode of the matrix changes ...
    cg.L.sb_cg_set_fuse_p(cg.ptr, 1 if second else 0)  # ... and so does the wish
    assert cg.fuse_p() == plan  # ... the running solve keeps its plan
    cg.run_iters(4)
    assert p.use_packed(first) == first
    cg.run_iters(iters)
    k = cg.finish()
    rr, pap = cg.history()
    assert equal_runs((k, rr, pap, cg.solution()), ref)
    cg.free(), p.free()


# ---- 4. the reference's own history through the mirror ------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,sigma", [("scs", 256), ("crs", 1)])
def test_seq_history_of_hpcg128_is_the_references(L, fmt, sigma):
    g = json.load(open(os.path.join(GOLDEN, "cg_hist_sp_ref.json")))["hpcg128"]
    assert g["itermax"] == 60
    shape = (128, 128, 128)
    want = fp64_all_row_programs(shape, fmt, sigma)
    p = problem(shape, fmt, sigma, mirror=True)
    assert p.all_row_programs() == want
    if fmt == "scs":
        assert want == 1
    if want:
        assert p.pack_info()["mode"] == 5  # every SpMV of the run is spmv_prog_f32
    (k, rr, pap, x), info = solve(p, g["itermax"], order="seq")
    assert info == (0, 0)
    assert k == g["k"]
    assert np.array_equal(bits(rr), bits([float(v) for v in g["rr"]]))
    assert np.array_equal(bits(pap), bits([float(v) for v in g["pAp"]]))
    p.free()


# ---- 5. driver ----------------------------------------------------------------------------------------------------------------
def test_the_sp_driver_runs_through_the_mirror():
    exe = os.path.join(BIN, "sparseBench-SCS-HIP-SP")
    cmd = [exe, "-x", "128", "-y", "128", "-z", "2", "-i", "30"]
    env = dict(os.environ, SB_DOT_ORDER="seq")
    env.pop("SB_SP_MIRROR", None), env.pop("SB_SP_MIRROR_REPORT", None)
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    on = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(env, SB_SP_MIRROR="1", SB_SP_MIRROR_REPORT="1"))
    assert plain.returncode == 0 and on.returncode == 0, (plain.stderr[-2000:], on.stderr[-2000:])
    assert "SP_MIRROR built=1 fmt=scs" in on.stderr, on.stderr[-2000:]
    assert "SP_MIRROR" not in plain.stderr
    res = lambda t: [ln for ln in t.splitlines() if "Residual" in ln or "iterations" in ln]
    assert len(res(on.stdout)) >= 3 and res(on.stdout) == res(plain.stdout), (on.stdout[-2000:], plain.stdout[-2000:])


# ---- 6. memory ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,fmt,sigma", SMALL + [((16, 16, 16), "scs", 1)])
def test_free_returns_the_device_memory(L, shape, fmt, sigma):
    problem(shape, fmt, sigma, mirror=True).free()  # (code objects, the layer's scratch: first use)
    before = device_free_bytes(L)
    p = problem(shape, fmt, sigma, mirror=True)
    assert p.pack_info()["mode"] == 5  # (built; a small matrix may fit the runtime's reserve, so free bytes need not drop)
    p.free()
    assert device_free_bytes(L) == before
