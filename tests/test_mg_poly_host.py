"""The CPU restatement of the Chebyshev-smoothed V-cycle (tests/precond_ref.py) pinned before the GPU is compared with
it: one V-cycle is the textbook one from scipy's pieces (A @ z, P.T @, P @) to rounding; the solve is PCG under that operator
(against scipy); one level is the polynomial plan bit for bit; the cycle's matrix is symmetric and positive definite; the launch count and
the byte model are the formulas of the contract; hostapi.mg_galerkin's matrices are P^T A P and survive their files bit for bit;
the iteration count does not grow from 16^3 to 32^3; tests/golden/mg_poly_hist.json holds what the restatement gives."""
import numpy as np
import pytest

import mg_poly_cases as cases
import pcg_ref
import precond_ref as ref
from conftest import load_json

EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def golden():
    return load_json("mg_poly_hist.json")


@pytest.fixture(scope="module")
def mg_golden():
    return load_json("mg_hist.json")


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("mg_poly")


def bits_equal(a, w):
    na = np.isnan(a)
    return np.array_equal(na, np.isnan(w)) and np.array_equal(a.view(np.uint64)[~na], w.view(np.uint64)[~na])


def textbook(hier, transfers):
    """the cycle as a function r -> z (level 0's device order) from scipy's pieces alone: the Chebyshev recurrence in its
    textbook form z += d, d = a d + b D^-1 (r - A z), with the restatement's scalars"""
    import scipy.sparse as sp
    lev = []
    for l, V in enumerate(hier.lev):
        A = pcg_ref.csr(V.g).tocsr()
        if V.op.o2n is not None:
            A = A[V.op.n2o][:, V.op.n2o].tocsr()
        e = dict(A=A, dinv=1.0 / A.diagonal(), c=V.smoother.c, steps=V.smoother.steps)
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

    def smooth(v, r, z):
        """`steps` steps from the guess z (None: from zero)"""
        c = v["c"]
        d = c["c1"] * v["dinv"] * (r if z is None else r - v["A"] @ z)
        z = d if z is None else z + d
        for j in range(2, v["steps"] + 1):
            d = c["a"][j] * d + c["b"][j] * (v["dinv"] * (r - v["A"] @ z))
            z = z + d
        return z

    def cycle(l, r):
        v = lev[l]
        z = smooth(v, r, None)
        if l == len(lev) - 1:
            return z
        zc = cycle(l + 1, v["omega"] * (v["P"].T @ (r - v["A"] @ z)))
        return smooth(v, r, z + v["P"] @ zc)

    return lambda r: cycle(0, np.asarray(r, dtype=np.float64))


@pytest.mark.parametrize("steps", [1, 2, 3])
@pytest.mark.parametrize("name", list(cases.SCIPY_CASES))
def test_cycle_is_the_textbook_cycle_and_symmetric(name, steps, tmp):
    """the contract and scipy's pieces round differently.  test_mg_fw_host.py takes 64 eps ||z|| per smoothing apply and per
    level's transfers; here a smoothing apply is `steps` steps, each an SpMV row of up to 27 terms and five more operations
    (32 eps), so two steps stand for one of those applies: 32 eps * steps * (2 L - 1) for the smoothings, 64 eps * (L - 1) for
    the transfers and the residual's SpMV"""
    pytest.importorskip("scipy")
    hier, transfers, op, b, dinv, eps = ref.build_case(ref.MGPOLY, dict(cases.SCIPY_CASES[name], steps=steps), tmp)
    bound = EPS * (32 * steps * (2 * hier.L - 1) + 64 * (hier.L - 1))
    want_of = textbook(hier, transfers)
    rng = np.random.RandomState(3)
    u, v = rng.standard_normal(hier.n), rng.standard_normal(hier.n)
    zu, zv = hier.apply(u)[0], hier.apply(v)[0]
    want = want_of(u)
    err = np.linalg.norm(zu - want) / np.linalg.norm(want)
    print("cycle against the textbook cycle", name, "steps", steps, "L", hier.L, err, "bound", bound)
    assert err <= bound
    a, c = float(u @ zv), float(v @ zu)
    print("symmetry", name, a, c, abs(a - c) / (np.linalg.norm(u) * np.linalg.norm(zv)))
    assert abs(a - c) <= bound * np.linalg.norm(u) * np.linalg.norm(zv)
    hier.free()


def scipy_gap(c, tmp):
    """as test_mg_fw_host.scipy_gap, with M the restated Chebyshev-smoothed cycle as a LinearOperator"""
    import scipy.sparse.linalg as sl
    hier, transfers, op, b, dinv, eps = ref.build_case(ref.MGPOLY, c, tmp)
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
    """bounded as test_mg_fw_host.py bounds its own: 10 x the gap tests/golden/mg_hist.json records for the injection cycle's case
    of the same name, which is rounding (< 1e-14); this cycle's own gap is recorded in mg_poly_hist.json"""
    pytest.importorskip("scipy")
    c = cases.SCIPY_CASES[name]
    gap, true_res, eps, k = scipy_gap(c, tmp)
    rec = mg_golden["scipy_gap"][name]
    print("scipy_gap", name, gap, "recorded here", golden["scipy_gap"][name], "bound 10 x", rec, "k", k, "true residual / eps", true_res / eps)
    assert 0.0 < rec < 1e-14
    assert gap <= 10.0 * rec
    assert k < c["itermax"]
    assert true_res <= 10.0 * eps


@pytest.mark.parametrize("matrix,fmt,sigma", [(("hpcg", 8), "crs", 1), (("dims", 7, 7, 6), "scs", 256), (("irregular", 12), "crs", 1)])
@pytest.mark.parametrize("coarse_steps", [1, 3])
def test_one_level_is_poly_ref_bit_for_bit(matrix, fmt, sigma, coarse_steps):
    """steps := coarse_steps: the only level is the last one"""
    c = dict(matrix=matrix, fmt=fmt, C=64, sigma=sigma, itermax=40, eps_rel=1e-10, coarse=[], steps=5, coarse_steps=coarse_steps,
             ratio=16.0)
    hier, transfers, op, b, dinv, eps = ref.build_case(ref.MGPOLY, c)
    assert hier.L == 1 and transfers == [] and hier.launches_per_body() == 5 + 2 * (coarse_steps - 1)
    plan = ref.poly(hier.lev[0].g, op, steps=coarse_steps)
    assert hier.lev[0].smoother.c == plan.lev[0].smoother.c
    assert hier.bytes() == (coarse_steps - 1) * (hier.lev[0].spmv_bytes() + 56.0 * hier.n) + 24.0 * hier.n
    for special in (False, True):
        r = ref.probe_vector(hier.n, 5, special)
        with np.errstate(all="ignore"):
            assert bits_equal(hier.apply(r)[0], plan.apply(r)[0])
    got, want = ref.solve(op, hier, b, dinv, 40, eps), ref.solve(op, plan, b, dinv, 40, eps)
    assert got["k"] == want["k"] > 5
    for key in ("rr", "rz", "pAp", "x"):
        assert bits_equal(got[key], want[key]), key
    hier.free()


@pytest.mark.parametrize("galerkin", [False, True])
@pytest.mark.parametrize("steps", [1, 2, 3])
def test_cycle_matrix_is_symmetric_and_positive_definite(steps, galerkin, tmp):
    """the dense matrix of the two-level cycle on the 8^3 stencil: the same polynomial before and after, so M^-1 is symmetric to
    rounding, and positive definite since every level's spectrum of D^-1 A lies in (0, lmax_l]"""
    pytest.importorskip("scipy")
    c = dict(matrix=("hpcg", 8), fmt="crs", C=64, sigma=1, levels=2, steps=steps, galerkin=galerkin)
    hier, transfers = ref.build_hierarchy(ref.MGPOLY, c, tmp)
    assert hier.L == 2 and hier.lev[0].transfer.omega == (1.0 if galerkin else 0.25)
    M = ref.dense_apply(hier)
    asym = np.abs(M - M.T).max() / np.abs(M).max()
    w = np.linalg.eigvalsh((M + M.T) * 0.5)
    print("steps", steps, "galerkin", galerkin, "asymmetry", asym, "eigenvalues of M^-1 in", w[0], w[-1])
    assert asym <= 64 * EPS * (3 * steps + 1)
    assert w[0] > 0.0
    for V in hier.lev:  # the premise: lambda(D^-1 A) in (0, lmax]
        A = pcg_ref.csr(V.g).toarray()
        sd = np.sqrt(1.0 / np.diag(A))
        lam = np.linalg.eigvalsh(sd[:, None] * A * sd[None, :])
        assert 0.0 < lam[0] and lam[-1] <= V.smoother.c["lmax"]
    hier.free()


@pytest.mark.parametrize("L,steps,coarse_steps,want", [(4, 1, None, 23), (4, 2, None, 37), (3, 3, 1, 33), (2, 16, 16, 101), (1, 2, 4, 11)])
def test_launch_count_is_the_contracts(L, steps, coarse_steps, want, tmp):
    """4 + (L - 1) (4 steps + 2) + 2 coarse_steps - 1, plus 1 where the SpMV has no fused dot: 23 at steps = 1, L = 4 and 37 at the
    defaults, where the full-weighting cycle with Gauss-Seidel sweeps has 120"""
    c = dict(matrix=("hpcg", 16), fmt="crs", C=64, sigma=1, levels=L, steps=steps, coarse_steps=coarse_steps)
    hier, transfers = ref.build_hierarchy(ref.MGPOLY, c, tmp)
    cs = steps if coarse_steps is None else coarse_steps
    assert hier.L == L and hier.launches_per_body() == 4 + (L - 1) * (4 * steps + 2) + 2 * cs - 1 == want
    assert hier.launches_per_body(fused_dot=False) == want + 1
    hier.free()


@pytest.mark.parametrize("fmt,C,sigma", [("crs", 64, 1), ("scs", 64, 256), ("scs", 4, 8)])
def test_byte_model_is_the_contracts_formula(fmt, C, sigma, tmp):
    """counted operation by operation in the restatement == the closed formula of DESIGN 4.16 and sbhip.h; integers in doubles"""
    for steps, cs in ((1, 1), (2, 2), (3, 1), (2, 5)):
        c = dict(matrix=("dims", 12, 8, 20), fmt=fmt, C=C, sigma=sigma, levels=3, steps=steps, coarse_steps=cs)
        hier, transfers = ref.build_hierarchy(ref.MGPOLY, c, tmp)
        want = 0.0
        for V in hier.lev[:-1]:
            want += 2 * steps * V.spmv_bytes() + (2 * (steps - 1) * 56.0 + 48.0 + 24.0) * V.n
            want += V.transfer.bytes() + 32.0 * V.n + 16.0 * V.transfer.nc
        last = hier.lev[-1]
        want += (cs - 1) * (last.spmv_bytes() + 56.0 * last.n) + 24.0 * last.n
        assert hier.bytes() == want and want == int(want)
        hier.free()
    # the structures: 12 B per padded element, 64 row lengths and 12 B per chunk; P^T of 12 x 8 x 20 has 240 rows, 27 entries at most
    V = ref.build_hierarchy(ref.MGPOLY, dict(matrix=("dims", 12, 8, 20), fmt="crs", C=64, sigma=1, levels=2), tmp)[0].lev[0]
    T = V.transfer
    assert T.nc == 240 and int(T.PT[0].max()) == 27 and int(T.P[0].max()) == 8
    assert V.spmv_bytes() == 12.0 * int(V.g.rowPtr[V.g.nr]) + 4.0 * 1921 + 16.0 * 1920


def test_mg_galerkin_is_pt_a_p_and_survives_its_files(tmp):
    sp = pytest.importorskip("scipy.sparse")
    from sparsebench_amd import hostapi
    p = hostapi.Problem("generate", 8, 8, 8, fmt="crs", upload=False)
    col, val = p.gm_entries()
    A = sp.csr_matrix((val, col.astype(np.int64), p.array("rowPtr").astype(np.int64)), shape=(512, 512)).toarray()
    d = tmp / "galerkin"
    d.mkdir()
    coarse = hostapi.mg_galerkin(p, levels=3, directory=d)
    assert [q.nr for q, _, _ in coarse] == [64, 8] and [w for _, _, w in coarse] == [1.0, 1.0]
    assert sorted(f.name for f in d.iterdir()) == ["level1.mtx", "level2.mtx"]
    dims = (8, 8, 8)
    for q, P, _ in coarse:
        ptr, cl, vl = ref.trilinear(dims)
        assert np.array_equal(P[0], ptr) and np.array_equal(P[1], cl) and np.array_equal(P[2], vl)
        Pd = sp.csr_matrix((vl, cl, ptr), shape=(len(ptr) - 1, q.nr)).toarray()
        A = Pd.T @ A @ Pd  # exact: the weights are powers of two and the stencil's values small integers
        qc, qv = q.gm_entries()
        qp = q.array("rowPtr").astype(np.int64)
        got = sp.csr_matrix((qv, qc.astype(np.int64), qp), shape=(q.nr, q.nr))
        assert np.array_equal(got.toarray(), A) and np.array_equal(A, A.T)
        assert got.nnz == np.count_nonzero(A) and np.all(qv != 0.0)  # exact zeros dropped
        for i in range(q.nr):
            assert np.all(np.diff(qc[qp[i]:qp[i + 1]].astype(np.int64)) > 0)  # sorted columns
        assert q.fmt == "crs" and q.filename.endswith(".mtx")
        dims = tuple(v // 2 for v in dims)
    # 17 significant digits bring every double back: a matrix whose values are not short decimals, through mg_galerkin's writer
    g = pcg_ref.gmatrix(("scaled", 8), tmp)
    S = pcg_ref.csr(g)
    Pt = ref.trilinear((8, 8, 8))
    gc, Ac = ref.galerkin_gmatrix(S, sp.csr_matrix((Pt[2], Pt[1], Pt[0]), shape=(512, 64)))
    path = str(d / "scaled.mtx")
    hostapi._write_mtx(path, Ac)
    q = hostapi.Problem(path, fmt="crs", upload=False)
    assert bits_equal(q.gm_entries()[1], Ac.data) and np.array_equal(q.gm_entries()[0], Ac.indices)
    q.free(), gc.free(), g.free()
    for q, _, _ in coarse:
        q.free()
    p.free()
    for bad in (hostapi.Problem("irregular", 4, 4, 4, fmt="crs", upload=False),):
        with pytest.raises(ValueError, match="needs the grid"):
            hostapi.mg_galerkin(bad)
        bad.free()


def count(c, tmp):
    hier, transfers, op, b, dinv, eps = ref.build_case(ref.MGPOLY, c, tmp)
    k = ref.solve(op, hier, b, dinv, c["itermax"], eps)["k"]
    L = hier.L
    hier.free()
    return k, L


def test_iteration_count_does_not_grow_with_the_grid(tmp, golden):
    """the claim the feature stands on, at eps = 1e-10 ||b||, steps = 2, ratio = 4, the deepest hierarchy: with Galerkin coarse
    operators k at 32^3 <= k at 16^3 + 2 and both <= 10; with the regenerated hierarchy at omega = 0.25 both <= 13"""
    pytest.importorskip("scipy")
    k = {}
    for name, c in cases.COUNT_CASES.items():
        k[name], L = count(c, tmp)
        print(name, "k", k[name], "L", L, "recorded", golden["counts"][name])
        assert L == 4 and golden["counts"][name] == dict(k=k[name], L=L)
    assert k["hpcg32_galerkin"] <= k["hpcg16_galerkin"] + 2 and max(k["hpcg16_galerkin"], k["hpcg32_galerkin"]) <= 10
    assert max(k["hpcg16_regenerated"], k["hpcg32_regenerated"]) <= 13


@pytest.mark.parametrize("n", [16, 32])
def test_the_count_table_of_the_design_document(n, tmp, golden):
    """DESIGN 4.16's table (Jacobi, the polynomial, the regenerated hierarchy at omega = 1/2 and 1/4, the Galerkin one, steps 1 / 2 / 3)
    is precond_ref.count_table's, recorded by the golden's maker; 16^3 and 32^3 are recomputed here, 64^3 (minutes) only by the maker"""
    pytest.importorskip("scipy")
    assert ref.count_table(n) == golden["table"][str(n)]
    assert set(golden["table"]) == {"16", "32", "64"}
    row = golden["table"]["64"]
    assert row["galerkin"][1] == golden["table"]["16"]["galerkin"][1]  # as recorded: two steps, the same count at 16^3 and 64^3


def golden_record(out):
    rec = pcg_ref.record(out)
    rec["L"], rec["rows"] = int(out["L"]), [int(v) for v in out["rows"]]
    rec["coeffs"] = [[float(v).hex() for v in level] for level in out["coeffs"]]
    rec["intervals"] = [[float(v).hex() for v in level] for level in out["intervals"]]
    rec["launches"], rec["bytes"] = int(out["launches"]), float(out["bytes"])
    return rec


@pytest.mark.parametrize("name", cases.SMALL)
def test_the_committed_golden_is_what_the_restatement_gives(name, tmp, golden):
    pytest.importorskip("scipy")
    assert golden_record(ref.run_case(ref.MGPOLY, cases.CASES[name], tmp)) == golden["cases"][name]
    assert set(golden["cases"]) == set(cases.CASES)
