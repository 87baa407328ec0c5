"""The block-vector kernels of batched CG alone: block_vec_k<NV, 0|1|2>, cgb_update_p<NV> and cgb_x_finalize<NV>
for NV in {2, 4, 8}, through the blocking entries that launch them with the loop's own launch functions.  Column c of every
kernel == the oracle's single-vector operation on column c, BIT FOR BIT (where a value is NaN, only the NaN positions are
compared): the level-1 values are po.ddot_partials, the vector updates po.waxpby, every total po.reduce_final == po.ddot_tree.

Sizes: one lane, one row pair, one span, the partial and the full group, odd sizes, several groups per workgroup, and the first
size past the grid's cap at which a wave takes a SECOND grid-stride trip that ends in a partial odd group -- taken from the
launch the library reports (sb_block_vec_launch, sb_cgb_rows_launch) and printed, never written down here.  Inputs: NaN, +-Inf,
-0.0 and subnormals at distinct rows of distinct columns and vectors, one column per case free of NaN / Inf, every device
array between sentinels (rows at or behind n are never read: the sentinels would change the dots).  Masks: every subset of
stopped (and owed) columns at the narrow widths, five patterns at the wide ones; a column that is masked keeps its BITS, NaN
payloads included, and its level-1 slots keep the sentinel.

cgb_scalar_k has no entry here: its paths are reached by tests/test_gpu_batch_cg.py (several columns exiting in one launch --
columns 3..7 at nv = 8 --, a zero column, the NaN exit)."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po

from sparsebench_amd.capi import DeviceVector
from test_gpu_bicgstab_kernels import SENTINEL, Guarded, same, specials

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDTHS = [2, 4, 8]
SMALL = [1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1430, 4097]
SIZES = SMALL + ["second_trip"]
# exactly representable, distinct per column
NALPHA = [-0.37109375, 1.2890625, -0.8203125, 0.6484375, -1.5390625, 0.2265625, -2.0078125, 0.9140625]
BETA = [0.4140625, -1.1171875, 0.7421875, 1.9609375, -0.2890625, 0.5859375, -0.6796875, 1.3359375]
ALPHA = [1.0546875, -0.4609375, 0.1953125, -1.7265625, 0.8828125, 2.3203125, -0.9765625, 0.3515625]


def launch(fn, n):
    out = np.zeros(3, dtype=np.uint32)
    fn(n, out.ctypes.data)
    assert int(out[1]) == 256 and int(out[2]) >= 1
    return int(out[0])


@pytest.fixture(scope="module")
def bv_sizes(gpu):
    """block_vec_k: a wave per 256-row group, four waves per workgroup; one full group more than the capped grid has waves,
    then 257 rows: the groups `waves` and `waves + 1` are second trips, the last one partial and odd"""
    cap = launch(gpu.sb_block_vec_launch, 0x7FFFFF00)
    n = 256 * (cap * 4) + 257
    assert launch(gpu.sb_block_vec_launch, n) == cap
    assert launch(gpu.sb_block_vec_launch, 1) == 1 and launch(gpu.sb_block_vec_launch, 4097) == min(cap, 5)
    print("block_vec_k: grid cap", cap, "workgroups; second grid-stride trip with a partial last group at n =", n)
    return dict({s: s for s in SMALL}, second_trip=n)


@pytest.fixture(scope="module")
def row_sizes(gpu):
    """cgb_update_p / cgb_x_finalize: a thread per row; one full workgroup more than the capped grid, then 257 rows"""
    cap = launch(gpu.sb_cgb_rows_launch, 0x7FFFFF00)
    n = 256 * cap + 257
    assert launch(gpu.sb_cgb_rows_launch, n) == cap
    assert launch(gpu.sb_cgb_rows_launch, 1) == 1 and launch(gpu.sb_cgb_rows_launch, 4097) == min(cap, 17)
    print("row kernels: grid cap", cap, "workgroups; second strip ending in a partial workgroup at n =", n)
    return dict({s: s for s in SMALL}, second_trip=n)


def block_columns(n, nv, seed, count, clean):
    """`count` block vectors of n rows as lists of nv columns: column c comes from specials(seed + c) and is rotated by 5 c rows,
    so kind j of vector w sits at different rows in different columns; the columns in `clean` hold no NaN / Inf"""
    vecs = [[] for _ in range(count)]
    for c in range(nv):
        for w, v in enumerate(specials(n, seed + c, count)):
            v = np.roll(v, (5 * c) % n)
            if c in clean:
                v[~np.isfinite(v)] = 1.5
            vecs[w].append(np.ascontiguousarray(v))
    return vecs


def interleave(cols):
    return np.stack(cols, axis=1).reshape(-1)  # element (row, c) at [row * nv + c]


def column(flat, nv, c):
    return np.ascontiguousarray(flat.reshape(-1, nv)[:, c])


def kept(got, orig, what):
    """the same bits, NaN payloads included"""
    a, b = np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(orig).view(np.uint64)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, (what, "changed at", int(bad[0]), got[bad[0]], orig[bad[0]])


def patterns(nv, exhaustive):
    """0 / 1 per column: every subset, or none, all, all but one, one, alternating"""
    if exhaustive:
        return [list(m) for m in itertools.product((0, 1), repeat=nv)]
    all_but_one, one = [1] * nv, [0] * nv
    all_but_one[nv - 2], one[1] = 0, 1
    return [[0] * nv, [1] * nv, all_but_one, one, [c % 2 for c in range(nv)]]


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def lib_level1(L, n, a, b):
    """the library's single-vector path: sb_ddot_partials' four values per 256 rows, combined ((q0 + q1) + q2) + q3"""
    m = (n + 255) // 256
    da, db, dq = DeviceVector.from_host(a), DeviceVector.from_host(b), DeviceVector.from_host(np.full(4 * m, SENTINEL))
    L.sb_ddot_partials(n, da.ptr, db.ptr, dq.ptr)
    q = dq.get().reshape(m, 4)
    for d in (da, db, dq):
        d.free()
    with np.errstate(all="ignore"):
        return ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]


def check_block_vec(L, op, nv, n, A, B, R, stop=None, single_path=False, coeff=NALPHA):
    """one launch of block_vec_k<nv, op> on the columns A, B (ops 0, 2) / A, R (op 1), everything asserted; returns R's columns"""
    nG = (n + 255) // 256
    what = ("block_vec", op, nv, n, stop)
    stop = [0] * nv if stop is None else stop
    nalpha = [np.nan if stop[c] else coeff[c] for c in range(nv)]
    dA, dl = Guarded(interleave(A)), Guarded(n=nv * nG)
    dB = Guarded(interleave(B)) if op != 1 else None
    dR = Guarded(interleave(R)) if op == 1 else Guarded(n=n * nv) if op == 2 else None
    na, st = f64(nalpha), i32(stop)
    L.sb_block_vec_native(op, nv, n, dA.ptr, dB.ptr if dB else None, dR.ptr if dR else None, na.ctypes.data if op == 1 else None,
                          st.ctypes.data if op == 1 else None, dl.ptr)
    l1 = dl.get((what, "l1")).reshape(nv, nG)  # exactly nv * nG values between the sentinels
    kept(dA.get((what, "A")), interleave(A), (what, "A untouched"))
    if dB:
        kept(dB.get((what, "B")), interleave(B), (what, "B untouched"))
    got_R = dR.get((what, "R")) if dR else None
    out = []
    for c in range(nv):
        if op == 0:
            x, y = A[c], B[c]
        elif op == 1 and stop[c]:
            kept(column(got_R, nv, c), R[c], (what, c, "a stopped column's r"))
            assert np.all(l1[c] == SENTINEL), (what, c, "a stopped column's level-1 values were written")
            out.append(R[c])
            continue
        else:
            x = y = po.waxpby(1.0, R[c], nalpha[c], A[c]) if op == 1 else po.waxpby(1.0, A[c], -1.0, B[c])
            same(column(got_R, nv, c), x, (what, c, "r"))
            out.append(x)
        want = po.ddot_partials(x, y)
        assert len(want) == nG
        same(l1[c], want, (what, c, "level-1 values"))
        same([po.reduce_final(l1[c])], [po.ddot_tree(x, y)], (what, c, "total"))
        if op == 0 and single_path:
            same(l1[c], lib_level1(L, n, x, y), (what, c, "the single-vector path's level-1 values"))
        # a column that is finite (inputs and coefficient) stays finite: nothing came over from a neighbour
        if all(np.isfinite(v[c]).all() for v in (A, B if op != 1 else R)) and np.isfinite(nalpha[c]):
            assert np.isfinite(l1[c]).all() and (op == 0 or np.isfinite(column(got_R, nv, c)).all()), (what, c, "not finite")
    for d in (dA, dB, dR, dl):
        if d:
            d.free()
    return out


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("nv", WIDTHS)
def test_block_vec_values_all_columns_live(gpu, bv_sizes, nv, size):
    n = bv_sizes[size]
    A, B, R = block_columns(n, nv, 1000 + 10 * nv, 3, {(n // 3) % nv})
    check_block_vec(gpu, 0, nv, n, A, B, None, single_path=True)
    check_block_vec(gpu, 2, nv, n, A, B, None)
    check_block_vec(gpu, 1, nv, n, A, None, R)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("nv", WIDTHS)
def test_block_vec_update_r_masks(gpu, bv_sizes, nv, size):
    """op 1 under every subset of stopped columns (nv = 2, 4) / the five patterns (nv = 8); at the second-trip size one mixed
    mask.  A stopped column has a NaN -alpha: its r keeps its bits all the same, its level-1 slots keep the sentinel"""
    n = bv_sizes[size]
    A, R = block_columns(n, nv, 2000 + 10 * nv, 2, {(n // 5) % nv})
    masks = [[(c + 1) % 2 for c in range(nv)]] if size == "second_trip" else patterns(nv, nv <= 4)
    for stop in masks:
        check_block_vec(gpu, 1, nv, n, A, None, R, stop=stop)


@pytest.mark.parametrize("n", [1, 65, 257, 513, 4097])
@pytest.mark.parametrize("nv", WIDTHS)
def test_block_vec_update_r_with_an_infinite_alpha(gpu, nv, n):
    """p . Ap == 0 makes -alpha infinite on a column that is still live: its r becomes +-Inf in every row and r . r is +Inf, not
    NaN -- the lanes at or behind n add +0.0, not the square of 0.0 + Inf * 0.0.  No entry of Ap is a zero here"""
    rng = np.random.default_rng(100 * nv + n)
    A = [rng.standard_normal(n) + 4.0 * np.sign(rng.standard_normal(n)) for _ in range(nv)]
    R = [rng.standard_normal(n) for _ in range(nv)]
    coeff = [(np.inf, -np.inf, NALPHA[2])[c % 3] for c in range(nv)]
    out = check_block_vec(gpu, 1, nv, n, A, None, R, coeff=coeff)
    for c in range(nv):
        if c % 3 != 2:  # (check_block_vec has compared the level-1 values and the total with these)
            assert np.isinf(out[c]).all() and po.ddot_tree(out[c], out[c]) == np.inf
        else:
            assert np.isfinite(out[c]).all()


def check_update_p(L, nv, n, R, P, X, stop, pend, which):
    """one launch of cgb_update_p<nv>; coefficients that must not be read are NaN.  Returns the columns of P and X it left"""
    what = ("update_p", nv, n, "stop", stop, "x_pending", pend, "which", which)
    live = [not s for s in stop]
    owed = [which == 0 and live[c] and bool(pend[c]) for c in range(nv)]
    beta = [BETA[c] if which == 0 and live[c] else np.nan for c in range(nv)]
    alpha = [ALPHA[c] if owed[c] else np.nan for c in range(nv)]
    dR, dP, dX = Guarded(interleave(R)), Guarded(interleave(P)), Guarded(interleave(X))
    b, a, st, pe = f64(beta), f64(alpha), i32(stop), i32(pend)
    L.sb_cgb_update_p_native(nv, n, dR.ptr, dP.ptr, dX.ptr, b.ctypes.data, a.ctypes.data, st.ctypes.data, pe.ctypes.data, which)
    got_P, got_X = dP.get((what, "P")), dX.get((what, "X"))
    kept(dR.get((what, "R")), interleave(R), (what, "R untouched"))
    if not any(owed):
        kept(got_X, interleave(X), (what, "nothing owed: X"))
    out_P, out_X = [], []
    for c in range(nv):
        if owed[c]:  # from the OLD p
            out_X.append(po.waxpby(1.0, X[c], alpha[c], P[c]))
            same(column(got_X, nv, c), out_X[c], (what, c, "x"))
        else:
            out_X.append(X[c])
            kept(column(got_X, nv, c), X[c], (what, c, "x of a column that is not owed"))
        if live[c]:
            out_P.append(po.waxpby(1.0, R[c], beta[c], P[c]) if which == 0 else po.waxpby(1.0, R[c], 0.0, R[c]))
            same(column(got_P, nv, c), out_P[c], (what, c, "p"))
        else:
            out_P.append(P[c])
            kept(column(got_P, nv, c), P[c], (what, c, "p of a stopped column"))
        if all(np.isfinite(v[c]).all() for v in (R, P, X)):
            assert np.isfinite(column(got_P, nv, c)).all() and np.isfinite(column(got_X, nv, c)).all(), (what, c, "not finite")
    for d in (dR, dP, dX):
        d.free()
    return out_P, out_X


def check_x_finalize(L, nv, n, X, P, pend, alpha=None):
    what = ("x_finalize", nv, n, "x_pending", pend)
    alpha = [ALPHA[c] if pend[c] else np.nan for c in range(nv)] if alpha is None else alpha
    dX, dP = Guarded(interleave(X)), Guarded(interleave(P))
    a, pe = f64(alpha), i32(pend)
    L.sb_cgb_x_finalize_native(nv, n, dX.ptr, dP.ptr, a.ctypes.data, pe.ctypes.data)
    got_X = dX.get((what, "X"))
    kept(dP.get((what, "P")), interleave(P), (what, "P untouched"))
    if not any(pend):
        kept(got_X, interleave(X), (what, "nothing owed: X"))
    out = []
    for c in range(nv):
        if pend[c]:
            out.append(po.waxpby(1.0, X[c], alpha[c], P[c]))
            same(column(got_X, nv, c), out[c], (what, c, "x"))
        else:
            out.append(X[c])
            kept(column(got_X, nv, c), X[c], (what, c, "x of a column that is not owed"))
        if all(np.isfinite(v[c]).all() for v in (P, X)):
            assert np.isfinite(column(got_X, nv, c)).all(), (what, c, "not finite")
    dX.free(), dP.free()
    return out


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("nv", WIDTHS)
def test_update_p_masks(gpu, row_sizes, nv, size):
    """which in {0, 1} x stopped columns x owed columns: every subset at nv = 2, the five patterns at nv = 4 and 8; at the
    second-strip size one mixed pair per form"""
    n = row_sizes[size]
    R, P, X = block_columns(n, nv, 3000 + 10 * nv, 3, {(n // 7) % nv})
    if size == "second_trip":
        combos = [([c % 2 for c in range(nv)], [1] * (nv - 1) + [0])]
    else:
        combos = list(itertools.product(patterns(nv, nv == 2), patterns(nv, nv == 2)))
    for stop, pend in combos:
        for which in (0, 1):
            check_update_p(gpu, nv, n, R, P, X, stop, pend, which)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("nv", WIDTHS)
def test_x_finalize_masks(gpu, row_sizes, nv, size):
    n = row_sizes[size]
    X, P = block_columns(n, nv, 4000 + 10 * nv, 2, {(n // 11) % nv})
    masks = [[(c + 1) % 2 for c in range(nv)], [0] * nv] if size == "second_trip" else patterns(nv, nv <= 4)
    for pend in masks:
        check_x_finalize(gpu, nv, n, X, P, pend)


@pytest.mark.parametrize("nv", WIDTHS)
def test_x_left_alone_by_update_p_is_finalized_exactly_once(gpu, nv):
    """column 1 has stopped with its x update owing: the p update of the columns still live leaves its x and p alone, the
    finalize applies alpha p to it once, and to it alone"""
    n = 513
    R, P, X = block_columns(n, nv, 5000 + nv, 3, {0})
    stop, pend = [0] * nv, [1] * nv
    stop[1] = 1
    P1, X1 = check_update_p(gpu, nv, n, R, P, X, stop, pend, 0)
    kept(X1[1], X[1], "x of the stopped column")
    kept(P1[1], P[1], "p of the stopped column")
    only = [int(c == 1) for c in range(nv)]
    X2 = check_x_finalize(gpu, nv, n, X1, P1, only)
    same(X2[1], po.waxpby(1.0, X[1], ALPHA[1], P[1]), "x of the stopped column, finalized once")
    for c in range(nv):
        if c != 1:
            same(X2[c], po.waxpby(1.0, X[c], ALPHA[c], P[c]), ("x of live column", c))


@pytest.mark.parametrize("nv", WIDTHS)
def test_a_finite_column_stays_finite_whatever_its_neighbours_hold(gpu, nv):
    """every other column is NaN, +Inf and -Inf throughout (and has NaN coefficients where it is masked): the one finite column
    comes out finite and with the oracle's bits, from all five kernels, at every position in the row"""
    n = 513
    rng = np.random.default_rng(nv)
    bad = np.array([np.nan, np.inf, -np.inf])
    for good in range(nv):
        def vec(shift):
            return [rng.standard_normal(n) if c == good else np.roll(np.resize(bad, n), c + shift) for c in range(nv)]
        A, B, R, P, X = (vec(s) for s in range(5))
        for stop in ([0] * nv, [int(c != good) for c in range(nv)]):
            for op in (0, 1, 2):
                out = check_block_vec(gpu, op, nv, n, A, B if op != 1 else None, R if op == 1 else None, stop=stop if op == 1 else None)
                assert op == 0 or np.isfinite(out[good]).all()
            for which in (0, 1):
                for pend in ([1] * nv, [int(c == good) for c in range(nv)], [int(c != good) for c in range(nv)]):
                    out_P, out_X = check_update_p(gpu, nv, n, R, P, X, stop, pend, which)
                    assert np.isfinite(out_P[good]).all() and np.isfinite(out_X[good]).all()
        for pend in ([1] * nv, [int(c == good) for c in range(nv)], [int(c != good) for c in range(nv)]):
            assert np.isfinite(check_x_finalize(gpu, nv, n, X, P, pend)[good]).all()


CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from sparsebench_amd import capi
from sparsebench_amd.capi import DeviceVector
L = capi.init(0)
what = sys.argv[1]
nv, n = 4, 64
a, b, c = (DeviceVector.from_host(np.ones(n * nv + 2)) for _ in range(3))
l1 = DeviceVector.from_host(np.zeros(nv + 4))
z, zi = np.zeros(nv), np.zeros(nv, dtype=np.int32)
if what == "block_vec_b":
    L.sb_block_vec_native(0, nv, n, a.ptr, b.ptr + 8, None, None, None, l1.ptr)
elif what == "block_vec_r":
    L.sb_block_vec_native(1, nv, n, a.ptr, None, c.ptr + 8, z.ctypes.data, zi.ctypes.data, l1.ptr)
elif what == "update_p":
    L.sb_cgb_update_p_native(nv, n, a.ptr, b.ptr + 8, c.ptr, z.ctypes.data, z.ctypes.data, zi.ctypes.data, zi.ctypes.data, 0)
elif what == "x_finalize":
    L.sb_cgb_x_finalize_native(nv, n, a.ptr + 8, b.ptr, z.ctypes.data, zi.ctypes.data)
print("NOT REFUSED")
"""


@pytest.mark.parametrize("what,fn", [("block_vec_b", "sb_block_vec_native"), ("block_vec_r", "sb_block_vec_native"),
                                     ("update_p", "sb_cgb_update_p_native"), ("x_finalize", "sb_cgb_x_finalize_native")])
def test_refusals_of_a_block_vector_that_is_not_16_byte_aligned(gpu, what, fn):
    """host-side argument check: fatal with file:line before the kernel is launched"""
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT, what], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 1, (out.returncode, out.stderr.decode()[-1000:])
    err = out.stderr.decode()
    assert fn + ": block vectors must be 16-byte aligned" in err and "sbhip:" in err and "NOT REFUSED" not in out.stdout.decode()
