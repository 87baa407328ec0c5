"""The CPU restatement of the V-cycle with full-weighting transfers (tests/precond_ref.py) pinned before the GPU is
compared with it: the trilinear P is the host library's and scipy's kron of the 1-D operators; one level is the SGS plan bit for bit;
the vectorised cycle is the entry-by-entry cycle; one V-cycle is the textbook one (triangular solves, A @ z, P.T @ d, P @ zc) to
rounding and a symmetric operator; the solve is PCG under that operator (against scipy); a stored weight of 0.0 changes nothing;
the hierarchy counts in the natural row order, where injection's is idle: the depth changes the cycle and the iteration count
falls below the two sweeps'; tests/golden/mg_fw_hist.json holds what the restatement gives."""
import numpy as np
import pytest

import mg_fw_cases as cases
import pcg_ref
import precond_ref as ref
from conftest import load_json

EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def golden():
    return load_json("mg_fw_hist.json")


@pytest.fixture(scope="module")
def mg_golden():
    return load_json("mg_hist.json")


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("mg_fw")


def bits_equal(a, w):
    na = np.isnan(a)
    return np.array_equal(na, np.isnan(w)) and np.array_equal(a.view(np.uint64)[~na], w.view(np.uint64)[~na])


@pytest.mark.parametrize("dims", cases.TRILINEAR_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_trilinear_p_is_the_host_librarys_and_the_kron_of_the_1d_operators(dims):
    sp = pytest.importorskip("scipy.sparse")
    from sparsebench_amd import hostapi
    ptr, col, val = ref.trilinear(dims)
    got = hostapi.mg_trilinear(*dims)
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and got[2].dtype == np.float64
    assert np.array_equal(got[0], ptr) and np.array_equal(got[1], col) and np.array_equal(got[2], val)
    nx, ny, nz = dims
    n, nc = nx * ny * nz, n_coarse(dims)
    P = sp.csr_matrix((val, col, ptr), shape=(n, nc))

    def line(m):
        A = np.zeros((m, m // 2))
        for i in range(m):
            if i % 2 == 0:
                A[i, i // 2] = 1.0
            else:
                A[i, (i - 1) // 2] = 0.5
                if (i + 1) // 2 < m // 2:
                    A[i, (i + 1) // 2] = 0.5
        return sp.csr_matrix(A)

    K = sp.kron(line(nz), sp.kron(line(ny), line(nx))).tocsr()  # x fastest
    K.eliminate_zeros()  # (kron keeps the blocks' structural zeros)
    assert (P != K).nnz == 0 and P.nnz == K.nnz  # exactly: the weights are products of 1 and 1/2
    assert set(np.unique(val).tolist()) <= {1.0, 0.5, 0.25, 0.125} and np.all(np.diff(ptr) <= 8) and np.all(np.diff(ptr) >= 1)
    for i in range(n):
        assert np.all(np.diff(col[ptr[i]:ptr[i + 1]]) > 0)  # ascending coarse number
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    interior = ((x < nx - 1) & (y < ny - 1) & (z < nz - 1)).ravel()
    rows = np.asarray(P.sum(axis=1)).ravel()
    assert np.all(rows[interior] == 1.0) and np.all(rows[~interior] < 1.0)
    cz, cy, cx = np.meshgrid(np.arange(nz // 2), np.arange(ny // 2), np.arange(nx // 2), indexing="ij")
    colsum = np.asarray(P.sum(axis=0)).ravel()
    # per dimension a coarse index c >= 1 is fed by fine 2c - 1, 2c, 2c + 1: 1/2 + 1 + 1/2 = 2, the last coarse index included
    # (fine n - 1 is odd and 2c + 1 for c = n/2 - 1: what is dropped there is ITS half weight for the coarse point past the
    # grid, which is why the upper faces' ROW sums fall short of 1, above).  Coarse index 0 has no fine point below it: 1 + 1/2.
    # So a column sums to 8 wherever no coarse index is 0, and to exactly 8 * (3/4)^(number of zero indices) on the lower faces
    want = np.where(cx == 0, 1.5, 2.0) * np.where(cy == 0, 1.5, 2.0) * np.where(cz == 0, 1.5, 2.0)
    assert np.array_equal(colsum, want.ravel())
    assert np.all(colsum[((cx > 0) & (cy > 0) & (cz > 0)).ravel()] == 8.0) and np.all(colsum <= 8.0)


def n_coarse(dims):
    return (dims[0] // 2) * (dims[1] // 2) * (dims[2] // 2)


@pytest.mark.parametrize("matrix,fmt,sigma", [(("hpcg", 8), "crs", 1), (("dims", 7, 7, 6), "scs", 256), (("irregular", 12), "crs", 1)])
def test_one_level_is_sgs_bit_for_bit(matrix, fmt, sigma):
    c = dict(matrix=matrix, fmt=fmt, C=64, sigma=sigma, itermax=40, eps_rel=1e-10, coarse=[])
    hier, transfers, op, b, dinv, eps = ref.build_case(ref.MGFW, c)
    assert hier.L == 1 and transfers == [] and hier.launches() == 2 * hier.lev[0].smoother.nC - 1
    plan = ref.sgs(hier.lev[0].g, op)
    for special in (False, True):
        r = ref.probe_vector(hier.n, 5, special)
        assert bits_equal(hier.apply(r)[0], plan.apply(r, op.to_dev(dinv))[0])
    got, want = ref.solve(op, hier, b, dinv, 40, eps), ref.solve(op, plan, b, dinv, 40, eps)
    assert got["k"] == want["k"] > 5
    for key in ("rr", "rz", "pAp", "x"):
        assert bits_equal(got[key], want[key]), key
    hier.free()


def cycle_scalar(hier, transfers, l, r):
    """V(l, r) entry by entry, as the contract words it, from the transfers in original numbering"""
    V = hier.lev[l]
    p, n = V.smoother, V.n
    z = ref.apply_scalar(p, r, V.dinv)
    if l == hier.L - 1:
        return z
    d = np.zeros(n)
    for i in range(n):
        s = np.float64(r[i])
        for cj, a in zip(*p.lower(i)):
            s = s - a * z[cj]
        for cj, a in zip(*p.upper(i)):
            s = s - a * z[cj]
        d[i] = s - V.diag[i] * z[i]
    (ptr, col, val), omega = transfers[l]
    C = hier.lev[l + 1]
    fdev = (lambda i: i) if V.op.o2n is None else (lambda i: V.op.o2n[i])
    cdev = (lambda c: c) if C.op.o2n is None else (lambda c: C.op.o2n[c])
    s = np.zeros(C.n)
    for i in range(n):  # ascending original fine row: every coarse row's sum grows in that order
        for e in range(ptr[i], ptr[i + 1]):
            if val[e] != 0.0:
                s[cdev(col[e])] = s[cdev(col[e])] + val[e] * d[fdev(i)]
    zc = cycle_scalar(hier, transfers, l + 1, omega * s)
    for i in range(n):
        kept = [e for e in range(ptr[i], ptr[i + 1]) if val[e] != 0.0]
        if kept:
            s = np.float64(0.0)
            for e in kept:
                s = s + val[e] * zc[cdev(col[e])]
            z[fdev(i)] = z[fdev(i)] + s
    t = np.zeros(n)
    for c in range(p.nC):
        for i in p.rows[c]:
            s = np.float64(r[i])
            for cj, a in zip(*p.lower(i)):
                s = s - a * z[cj]
            t[i] = s
            for cj, a in zip(*p.upper(i)):
                s = s - a * z[cj]
            z[i] = s * V.dinv[i]
    for c in range(p.nC - 2, -1, -1):
        for i in p.rows[c]:
            s = np.float64(t[i])
            for cj, a in zip(*p.upper(i)):
                s = s - a * z[cj]
            z[i] = s * V.dinv[i]
    return z


@pytest.mark.parametrize("which", ["dims_4_4_4_L2", "dims_8_4_6_L2_permuted", "hand_made", "hand_made_permuted"])
def test_vectorised_cycle_is_the_entry_by_entry_cycle(which, tmp):
    c = {"dims_4_4_4_L2": dict(matrix=("dims", 4, 4, 4), fmt="crs", C=64, sigma=1, levels=2),
         "dims_8_4_6_L2_permuted": dict(matrix=("dims", 8, 4, 6), fmt="scs", C=64, sigma=256, levels=2),
         "hand_made": cases.hand_made_case(tmp), "hand_made_permuted": cases.hand_made_case(tmp, "scs", 256)}[which]
    hier, transfers = ref.build_hierarchy(ref.MGFW, c, tmp)
    assert hier.L == 2
    for special in (False, True):
        r = ref.probe_vector(hier.n, 7, special)
        z = hier.apply(r)[0]
        with np.errstate(all="ignore"):
            want = cycle_scalar(hier, transfers, 0, r)
        assert bits_equal(z, want)
        assert np.isnan(z).any() == special
    hier.free()


def textbook(hier, transfers):
    """the cycle as a function r -> z (level 0's device order) from scipy's pieces alone"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as sl
    lev = []
    for l, V in enumerate(hier.lev):
        A = pcg_ref.csr(V.g).tocsr()
        if V.op.o2n is not None:
            A = A[V.op.n2o][:, V.op.n2o].tocsr()
        perm = np.argsort(V.smoother.colour, kind="stable")
        B = A[perm][:, perm].tocsr()
        e = dict(A=A, perm=perm, d=B.diagonal(), DL=sp.tril(B, 0).tocsr(), DU=sp.triu(B, 0).tocsr(), Lo=sp.tril(B, -1).tocsr(),
                 Up=sp.triu(B, 1).tocsr())
        if l + 1 < hier.L:
            (ptr, col, val), e["omega"] = transfers[l]
            P = sp.csr_matrix((val, col, ptr), shape=(V.n, hier.lev[l + 1].n))
            C = hier.lev[l + 1]
            if V.op.o2n is not None:
                P = P[V.op.n2o]
            if C.op.o2n is not None:
                P = P[:, C.op.n2o]
            e["P"] = P.tocsr()
        lev.append(e)

    def cycle(l, r):
        v = lev[l]
        perm = v["perm"]
        z = np.empty(len(r))
        z[perm] = sl.spsolve_triangular(v["DU"], v["d"] * sl.spsolve_triangular(v["DL"], r[perm], lower=True), lower=False)
        if l == len(lev) - 1:
            return z
        zc = cycle(l + 1, v["omega"] * (v["P"].T @ (r - v["A"] @ z)))
        z = z + v["P"] @ zc
        z1 = sl.spsolve_triangular(v["DL"], r[perm] - v["Up"] @ z[perm], lower=True)
        z[perm] = sl.spsolve_triangular(v["DU"], r[perm] - v["Lo"] @ z1, lower=False)
        return z

    return lambda r: cycle(0, np.asarray(r, dtype=np.float64))


@pytest.mark.parametrize("name", list(cases.SCIPY_CASES))
def test_cycle_is_the_textbook_cycle_and_symmetric(name, tmp):
    """the contract and scipy's pieces round differently.  test_mg_host.py's bound for the injection cycle is test_sgs_host.py's
    for one smoothing apply, 64 eps ||z||, times the 2 L - 1 smoothing applies; this cycle adds per level but the last a full
    residual (a row of up to 27 terms: 27 eps), a restriction (up to 27 terms of weight <= 1, scaled: 28 eps) and a
    prolongation (up to 8 terms: 8 eps): 63 eps, taken as one more 64 eps each"""
    pytest.importorskip("scipy")
    hier, transfers, op, b, dinv, eps = ref.build_case(ref.MGFW, cases.SCIPY_CASES[name], tmp)
    bound = 64 * EPS * (2 * hier.L - 1 + hier.L - 1)
    want_of = textbook(hier, transfers)
    rng = np.random.RandomState(3)
    u, v = rng.standard_normal(hier.n), rng.standard_normal(hier.n)
    zu, zv = hier.apply(u)[0], hier.apply(v)[0]
    want = want_of(u)
    err = np.linalg.norm(zu - want) / np.linalg.norm(want)
    print("cycle against the textbook cycle", name, "L", hier.L, err, "bound", bound)
    assert err <= bound
    a, c = float(u @ zv), float(v @ zu)
    print("symmetry", name, a, c, abs(a - c) / (np.linalg.norm(u) * np.linalg.norm(zv)))
    assert abs(a - c) <= bound * np.linalg.norm(u) * np.linalg.norm(zv)
    hier.free()


def scipy_gap(c, tmp):
    """as test_mg_host.scipy_gap, with M the restated full-weighting cycle as a LinearOperator"""
    import scipy.sparse.linalg as sl
    hier, transfers, op, b, dinv, eps = ref.build_case(ref.MGFW, c, tmp)
    assert op.o2n is None
    ours = ref.solve(op, hier, b, dinv, c["itermax"], eps, keep_x=True)
    xs = ours["xs"]
    A = pcg_ref.csr(hier.lev[0].g)
    M = sl.LinearOperator(A.shape, matvec=lambda r: hier.apply(np.asarray(r, dtype=np.float64).ravel())[0], dtype=np.float64)
    theirs = []
    sl.cg(A, b, x0=np.zeros(len(b)), rtol=0.0, atol=0.0, maxiter=len(xs), M=M, callback=lambda xk: theirs.append(xk.copy()))
    assert len(theirs) == len(xs) >= 5
    gap = max(float(np.linalg.norm(a - t) / np.linalg.norm(a)) for a, t in zip(xs, theirs))
    true_res = float(np.linalg.norm(b - A @ ours["x"]))
    hier.free()
    return gap, true_res, eps, ours["k"]


@pytest.mark.parametrize("name", ["hpcg16_L4", "scaled16_over_hpcg8"])
def test_restatement_is_pcg_against_scipy(name, tmp, golden, mg_golden):
    """the bound is the injection cycle's: 10 x the gap tests/golden/mg_hist.json records for the case of the same name, which is
    rounding (< 1e-14); this cycle's own gap is recorded beside it in mg_fw_hist.json"""
    pytest.importorskip("scipy")
    c = cases.SCIPY_CASES[name]
    gap, true_res, eps, k = scipy_gap(c, tmp)
    rec = mg_golden["scipy_gap"][name]
    print("scipy_gap", name, gap, "recorded here", golden["scipy_gap"][name], "bound 10 x", rec, "k", k, "true residual / eps", true_res / eps)
    assert 0.0 < rec < 1e-14
    assert gap <= 10.0 * rec
    assert k < c["itermax"]
    assert true_res <= 10.0 * eps


def test_a_stored_weight_of_zero_changes_nothing(tmp):
    """the hand-made P stores a 0.0 in row 21 and leaves row 7 empty: the cycle and the solve with the 0.0 stored are those
    with it left out, bit for bit, also where 0.0 * inf would have made a NaN"""
    for fmt, sigma in (("crs", 1), ("scs", 256)):
        outs = []
        for store_zero in (True, False):
            c = cases.hand_made_case(tmp, fmt, sigma, store_zero)
            hier, transfers, op, b, dinv, eps = ref.build_case(ref.MGFW, c, tmp)
            P = transfers[0][0]
            assert P[0][cases.EMPTY_ROW + 1] == P[0][cases.EMPTY_ROW]
            assert (0.0 in P[2].tolist()) == store_zero
            zs = [hier.apply(ref.probe_vector(hier.n, 9, special))[0] for special in (False, True)]
            d, rc, zo = hier.probe(0, ref.probe_vector(130, 1, True), ref.probe_vector(130, 2, True), ref.probe_vector(65, 3, True))
            outs.append(zs + [d, rc, zo, ref.solve(op, hier, b, dinv, c["itermax"], eps)])
            hier.free()
        for a, w in zip(outs[0][:-1], outs[1][:-1]):
            assert bits_equal(a, w)
        assert outs[0][-1]["k"] == outs[1][-1]["k"] and bits_equal(outs[0][-1]["x"], outs[1][-1]["x"])
    # the empty row keeps its z through the prolongation, the sign of a zero included (z + (+0.0) would lose it)
    hier, transfers = ref.build_hierarchy(ref.MGFW, cases.hand_made_case(tmp), tmp)
    z = np.ones(130)
    z[cases.EMPTY_ROW] = z[8] = -0.0
    zo = hier.probe(0, np.zeros(130), z, np.zeros(65))[2]
    assert np.signbit(zo[cases.EMPTY_ROW]) and not np.signbit(zo[8]) and zo[8] == 0.0
    hier.free()


def test_in_the_natural_order_the_depth_changes_the_cycle(tmp):
    """what injection could not do (test_mg_host.py::test_in_the_natural_order_the_coarse_levels_are_idle): in CRS at 16^3 the
    cycle is not the two sweeps, and the cycles of three and of four levels differ"""
    zs = {}
    for L in (3, 4):
        hier, transfers = ref.build_hierarchy(ref.MGFW, dict(matrix=("hpcg", 16), fmt="crs", C=64, sigma=1, levels=L), tmp)
        r = np.random.RandomState(1).standard_normal(hier.n)
        zs[L] = hier.apply(r)[0]
        two = ref.TwoSweeps(hier.lev[0]).apply(r)[0]
        V = hier.lev[0]
        rc = V.transfer.restrict(V, r, V.smoother.pre(r)[0])
        print("L", L, "||rc|| / ||r||", np.linalg.norm(rc) / np.linalg.norm(r), "||V(r) - two sweeps|| / ||V(r)||",
              np.linalg.norm(zs[L] - two) / np.linalg.norm(zs[L]))
        assert np.linalg.norm(rc) > 1e-3 * np.linalg.norm(r) and np.linalg.norm(zs[L] - two) > 1e-4 * np.linalg.norm(zs[L])
        hier.free()
    assert not bits_equal(zs[3], zs[4]) and np.linalg.norm(zs[3] - zs[4]) > 1e-8 * np.linalg.norm(zs[4])


def count(c, tmp):
    hier, transfers, op, b, dinv, eps = ref.build_case(ref.MGFW, c, tmp)
    k = ref.solve(op, hier, b, dinv, c["itermax"], eps)["k"]
    L = hier.L
    hier.free()
    return k, L


@pytest.mark.parametrize("name", list(cases.COUNT_CASES))
def test_iteration_count_falls_below_the_two_sweeps(name, tmp, golden, mg_golden):
    """k to 1e-10 ||b||: Jacobi, SGS, the two sweeps and injection MG are tests/golden/mg_hist.json's (pinned by test_mg_host.py);
    the full-weighting cycle's is computed here.  Strictly fewer than the two sweeps in the natural order (hpcg16, hpcg32 in
    CRS); in Sell-64-256 the restatement shows the same, so it is asserted there too"""
    c = cases.COUNT_CASES[name]
    k, L = count(c, tmp)
    rec = golden["counts"][name]
    print(name, "k_mgfw", k, rec)
    assert {key: rec[key] for key in ("k_jacobi", "k_sgs", "k_two_sweeps", "k_mg", "L")} == mg_golden["counts"][name]
    assert rec["k_mgfw"] == k and L == rec["L"]
    assert k < rec["k_two_sweeps"] <= rec["k_sgs"] < rec["k_jacobi"]
    assert k < rec["k_mg"]


def golden_record(out):
    rec = pcg_ref.record(out)
    rec["nC"], rec["L"], rec["rows"] = [int(v) for v in out["nC"]], int(out["L"]), [int(v) for v in out["rows"]]
    return rec


@pytest.mark.parametrize("name", cases.SMALL)
def test_the_committed_golden_is_what_the_restatement_gives(name, tmp, golden):
    assert golden_record(ref.run_case(ref.MGFW, cases.CASES[name], tmp)) == golden["cases"][name]
    assert set(golden["cases"]) == set(cases.CASES)
