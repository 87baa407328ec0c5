"""The full-weighting transfers on the GPU without a solve: the three kernels each on its own through
sb_pcg_mg_fw_probe -- d = r - A z, rc = omega P^T d, z + P zc -- and one whole V-cycle through sb_pcg_apply_precond == the CPU
restatement (tests/precond_ref.py, pinned by tests/test_mg_fw_host.py) BIT FOR BIT, NaN equal to NaN, on vectors with +0.0, -0.0,
a denormal, an inf and a NaN in r, z and zc.  The shapes are mg_cases': 4^3 (8 coarse rows: one partial chunk of P^T),
34 x 6 x 10 (every colour ends in a partial chunk, so the one-launch residual crosses colour boundaries at partial chunks),
12 x 8 x 20 (odd coarse dimensions: dropped boundary weights where the coarse colouring is not the parity one), three and four
levels, every format; a caller's hierarchy with an empty row of P and a stored weight of 0.0.  One level is the SGS handle."""
import numpy as np
import pytest

import mg_fw_cases as cases
import pcg_ref
import precond_ref as ref
from sparsebench_amd import hostapi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("mg_fw_kernels")


def same(got, want, what):
    a, b = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), (what, "NaN positions differ", np.nonzero(na != nb)[0][:5])
    bad = np.nonzero((a.view(np.uint64) != b.view(np.uint64)) & ~na)[0]
    assert bad.size == 0, (what, "first difference at", int(bad[0]), a[bad[0]], b[bad[0]], "of", bad.size)


def fused_dot(p, fmt, C):
    return (fmt == "scs" and C == 64) or p.use_packed(5) == 5


def check_handle(s, p, hier, fmt, C, what):
    """levels, rows, colours, launches, every level's transfers on their own and two whole cycles against the restatement"""
    op = hier.lev[0].op
    assert s.precond() == "mgfw" and s.levels() == hier.L, (what, s.precond(), s.levels(), hier.L)
    assert [s.level_rows(l) for l in range(hier.L)] == [V.n for V in hier.lev], what
    assert [s.level_colours(l) for l in range(hier.L)] == [V.smoother.nC for V in hier.lev], what
    assert s.colours() == hier.lev[0].smoother.nC and np.array_equal(s.colouring(), op.to_orig(hier.lev[0].smoother.colour)), what
    apply_launches = sum(2 * (2 * V.smoother.nC - 1) + 3 for V in hier.lev[:-1]) + 2 * hier.lev[-1].smoother.nC - 1
    assert hier.launches() == apply_launches
    assert s.launches_per_body() == 6 + apply_launches + (0 if fused_dot(p, fmt, C) else 1), what
    for l in range(hier.L - 1):
        V, W = hier.lev[l], hier.lev[l + 1]
        for seed, special in ((3, False), (4, True)):
            r, z, zc = ref.probe_vector(V.n, seed, special), ref.probe_vector(V.n, seed + 10, special), ref.probe_vector(W.n, seed + 20, special)
            if special and V.n > 8:  # an inf in z beside rows that do not touch it, a NaN in zc
                z[5], zc[W.n // 2] = -np.inf, np.nan
            want = hier.probe(l, V.op.to_dev(r), V.op.to_dev(z), W.op.to_dev(zc))
            got = s.mg_fw_probe(l, r, z, zc)
            for name, g, w, o in zip(("d", "rc", "z_out"), got, want, (V.op, W.op, V.op)):
                same(g, o.to_orig(w), what + (l, name, "special" if special else "finite"))
    for seed, special in ((1, False), (2, True)):
        r = ref.probe_vector(hier.n, seed, special)
        want = op.to_orig(hier.apply(op.to_dev(r))[0])
        same(s.apply(r), want, what + ("cycle", "special" if special else "finite"))
        if hier.n > 5:
            assert np.isnan(want).any() == special
    assert s.precond_bytes() > 2 * 40.0 * hier.n and s.apply_ms(2) > 0.0


def check(matrix, levels, fmt, C, sigma, tmp):
    c = dict(matrix=matrix, fmt=fmt, C=C, sigma=sigma, levels=levels)
    hier, transfers = ref.build_hierarchy(ref.MGFW, c, tmp)
    assert hier.L == levels
    p = hostapi.Problem(*pcg_ref.problem_args(matrix, tmp), fmt=fmt, Cc=C, sigma=sigma)
    if sigma > 1:  # the restatement walks the device's own permutation
        op = hier.lev[0].op
        assert np.array_equal(p.array("oldToNewPerm"), op.o2n if op.o2n is not None else np.arange(p.nr))
    s = hostapi.PCG(p, precond="mgfw", levels=levels)
    check_handle(s, p, hier, fmt, C, (matrix, levels, fmt, C, sigma))
    s.free(), p.free(), hier.free()
    return hier


@pytest.mark.parametrize("fmt,C,sigma", cases.KERNEL_FORMATS)
@pytest.mark.parametrize("matrix,levels", cases.KERNEL_SHAPES, ids=lambda m: "_".join(str(v) for v in m) if isinstance(m, tuple) else "L%d" % m)
def test_transfers_and_one_cycle_equal_the_restatement(gpu, matrix, levels, fmt, C, sigma, tmp):
    hier = check(matrix, levels, fmt, C, sigma, tmp)
    rows = [V.n for V in hier.lev]
    if matrix == ("dims", 4, 4, 4):
        # one partial chunk of P^T; the corner-free row has 27 entries
        assert rows == [64, 8] and int(hier.lev[0].transfer.PT[0].max()) == 27
    if matrix == ("dims", 16, 16, 16):
        assert rows == [4096, 512, 64, 8]
    if matrix == ("dims", 12, 8, 20) and sigma == 1:
        assert rows == [1920, 240, 30]
    if matrix == ("dims", 34, 6, 10) and sigma == 1:
        assert all(len(r) % 64 for r in hier.lev[0].smoother.rows)  # every colour ends in a partial chunk
    ln = hier.lev[0].transfer.P[0]
    assert ln.min() >= 1 and ln.max() == 8  # chunk lengths of P vary between 1 and 8


def test_sell_4_8(gpu, tmp):
    matrix, levels = cases.SELL_4_8_SHAPE
    check(matrix, levels, "scs", 4, 8, tmp)


@pytest.mark.parametrize("fmt,sigma", [("crs", 1), ("scs", 1), ("scs", 256)])
def test_a_callers_hierarchy_with_an_empty_row_and_a_zero_weight(gpu, fmt, sigma, tmp):
    fine, coarse, P, omega = cases.hand_made(tmp)
    c = cases.hand_made_case(tmp, fmt, sigma)
    hier, transfers = ref.build_hierarchy(ref.MGFW, c, tmp)
    assert [V.n for V in hier.lev] == [130, 65] and omega == 0.5 and 0.0 in P[2].tolist()
    assert (hier.lev[0].transfer.P[0] == 0).sum() == 1  # the empty row
    p = hostapi.Problem(fine, 1, 1, 1, fmt=fmt, Cc=64, sigma=sigma)
    q = hostapi.Problem(coarse, 1, 1, 1, fmt=fmt, Cc=64, sigma=sigma)
    if fmt == "crs":  # as a scipy.sparse matrix, the stored 0.0 kept
        import scipy.sparse as sp
        given = sp.csr_matrix((P[2], P[1], P[0]), shape=(130, 65))
        assert given.nnz == len(P[2])
    else:
        given = P
    s = hostapi.PCG(p, precond="mgfw", coarse=[(q, given, omega)])
    check_handle(s, p, hier, fmt, 64, ("hand made", fmt, sigma))
    # the empty row's z goes through the prolongation untouched, the sign of its zero included
    z = np.ones(130)
    z[cases.EMPTY_ROW] = -0.0
    zo = s.mg_fw_probe(0, np.zeros(130), z, np.zeros(65))[2]
    assert zo[cases.EMPTY_ROW] == 0.0 and np.signbit(zo[cases.EMPTY_ROW])
    s.free(), q.free(), p.free(), hier.free()


@pytest.mark.parametrize("fmt,C,sigma", cases.KERNEL_FORMATS)
def test_one_level_is_the_sgs_handle(gpu, fmt, C, sigma):
    p = hostapi.Problem("generate", 10, 11, 13, fmt=fmt, Cc=C, sigma=sigma)
    s, m = hostapi.PCG(p, precond="sgs"), hostapi.PCG(p, precond="mgfw", levels=1)
    assert m.precond() == "mgfw" and m.levels() == 1
    assert m.level_rows(0) == p.nr and m.level_colours(0) == s.colours() == m.colours()
    assert m.launches_per_body() == s.launches_per_body() and m.precond_bytes() == s.precond_bytes()
    assert np.array_equal(m.colouring(), s.colouring())
    for seed, special in ((1, False), (2, True)):
        r = ref.probe_vector(p.nr, seed, special)
        same(m.apply(r), s.apply(r), (fmt, C, sigma, special))
    same(m.dinv(), s.dinv(), "dinv")
    m.free(), s.free(), p.free()
