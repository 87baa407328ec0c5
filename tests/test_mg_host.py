"""The CPU restatement of MG-preconditioned CG (tests/precond_ref.py) pinned before the GPU is compared with it: one
level is the SGS plan bit for bit; the vectorised cycle is the entry-by-entry cycle; one V-cycle is the textbook one (triangular
solves in colour order, a sparse A z, fancy-indexed injection) to rounding; the cycle is a symmetric operator; the solve is PCG
under that operator (against scipy); the geometric hierarchy's rule and injection map are the host library's; the iteration
count drops against SGS and Jacobi -- by as much as the two sweeps of level 0 alone give; in the natural row order the coarse
levels are idle bit for bit, in a permuted order they are not; tests/golden/mg_hist.json holds what the restatement gives."""
import numpy as np
import pytest

import mg_cases
import pcg_ref
import precond_ref as ref
from conftest import load_json

EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def golden():
    return load_json("mg_hist.json")


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("mg")


def bits_equal(a, w):
    na = np.isnan(a)
    return np.array_equal(na, np.isnan(w)) and np.array_equal(a.view(np.uint64)[~na], w.view(np.uint64)[~na])


@pytest.mark.parametrize("matrix,fmt,sigma", [(("hpcg", 8), "crs", 1), (("dims", 7, 7, 6), "scs", 256), (("irregular", 12), "crs", 1)])
def test_one_level_is_sgs_bit_for_bit(matrix, fmt, sigma):
    c = dict(matrix=matrix, fmt=fmt, C=64, sigma=sigma, itermax=40, eps_rel=1e-10, coarse=[])
    hier, f2cs, op, b, dinv, eps = ref.build_case(ref.MG, c)
    assert hier.L == 1 and f2cs == [] and hier.launches() == 2 * hier.lev[0].smoother.nC - 1
    plan = ref.sgs(hier.lev[0].g, op)
    for special in (False, True):
        r = ref.probe_vector(hier.n, 5, special)
        assert bits_equal(hier.apply(r)[0], plan.apply(r, op.to_dev(dinv))[0])
    got, want = ref.solve(op, hier, b, dinv, 40, eps), ref.solve(op, plan, b, dinv, 40, eps)
    assert got["k"] == want["k"] > 5
    for key in ("rr", "rz", "pAp", "x"):
        assert bits_equal(got[key], want[key]), key
    hier.free()


def cycle_scalar(hier, l, r):
    """V(l, r) entry by entry, as the contract words it"""
    V = hier.lev[l]
    p, n, fine = V.smoother, V.n, V.transfer and V.transfer.fine
    ptr, col, val = ref.device_rows(V.g, V.op)
    z = ref.apply_scalar(p, r, V.dinv)
    if l == hier.L - 1:
        return z
    rc = np.zeros(len(fine))
    for c, f in enumerate(fine):
        s = np.float64(r[f])
        for e in range(ptr[f], ptr[f + 1]):
            if val[e] != 0.0:
                s = s - val[e] * z[col[e]]
        rc[c] = s
    zc = cycle_scalar(hier, l + 1, rc)
    for c, f in enumerate(fine):
        z[f] = z[f] + zc[c]
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


def hand_made_case(tmp, fmt="crs", sigma=1):
    fine, coarse, f2c = mg_cases.hand_made(tmp)
    return dict(matrix=("file", fine), fmt=fmt, C=64, sigma=sigma, itermax=150, eps_rel=1e-10, coarse=[(("file", coarse), f2c)])


@pytest.mark.parametrize("which", ["dims_4_4_4_L2", "dims_8_4_6_L2_permuted", "hand_made", "hand_made_permuted"])
def test_vectorised_cycle_is_the_entry_by_entry_cycle(which, tmp):
    c = {"dims_4_4_4_L2": dict(matrix=("dims", 4, 4, 4), fmt="crs", C=64, sigma=1, levels=2),
         "dims_8_4_6_L2_permuted": dict(matrix=("dims", 8, 4, 6), fmt="scs", C=64, sigma=256, levels=2),
         "hand_made": hand_made_case(tmp), "hand_made_permuted": hand_made_case(tmp, "scs", 256)}[which]
    hier, f2cs = ref.build_hierarchy(ref.MG, c, tmp)
    assert hier.L == 2
    for special in (False, True):
        r = ref.probe_vector(hier.n, 7, special)
        z = hier.apply(r)[0]
        with np.errstate(all="ignore"):
            want = cycle_scalar(hier, 0, r)
        assert bits_equal(z, want)
        assert np.isnan(z).any() == special
    hier.free()


def textbook(hier):
    """the cycle as a function r -> z (level 0's device order) from scipy's pieces alone"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as sl
    lev = []
    for V in hier.lev:
        A = pcg_ref.csr(V.g).tocsr()
        if V.op.o2n is not None:
            A = A[V.op.n2o][:, V.op.n2o].tocsr()
        perm = np.argsort(V.smoother.colour, kind="stable")
        B = A[perm][:, perm].tocsr()
        lev.append(dict(A=A, perm=perm, d=B.diagonal(), DL=sp.tril(B, 0).tocsr(), DU=sp.triu(B, 0).tocsr(), Lo=sp.tril(B, -1).tocsr(),
                        Up=sp.triu(B, 1).tocsr(), fine=V.transfer and V.transfer.fine))

    def cycle(l, r):
        v = lev[l]
        perm = v["perm"]
        z = np.empty(len(r))
        z[perm] = sl.spsolve_triangular(v["DU"], v["d"] * sl.spsolve_triangular(v["DL"], r[perm], lower=True), lower=False)
        if l == len(lev) - 1:
            return z
        zc = cycle(l + 1, (r - v["A"] @ z)[v["fine"]])
        z[v["fine"]] += zc
        z1 = sl.spsolve_triangular(v["DL"], r[perm] - v["Up"] @ z[perm], lower=True)
        z[perm] = sl.spsolve_triangular(v["DU"], r[perm] - v["Lo"] @ z1, lower=False)
        return z

    return lambda r: cycle(0, np.asarray(r, dtype=np.float64))


def scipy_case(name, tmp):
    return ref.build_case(ref.MG, mg_cases.SCIPY_CASES[name], tmp)


@pytest.mark.parametrize("name", list(mg_cases.SCIPY_CASES))
def test_cycle_is_the_textbook_cycle_and_symmetric(name, tmp):
    """the contract and scipy's solves round differently: test_sgs_host.py's bound for one smoothing apply, 64 eps ||z||, times the
    2 L - 1 smoothing applies of the cycle"""
    pytest.importorskip("scipy")
    hier, f2cs, op, b, dinv, eps = scipy_case(name, tmp)
    bound = 64 * EPS * (2 * hier.L - 1)
    want_of = textbook(hier)
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
    """as test_sgs_host.scipy_gap, with M the restated cycle as a LinearOperator"""
    import scipy.sparse.linalg as sl
    hier, f2cs, op, b, dinv, eps = ref.build_case(ref.MG, c, tmp)
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
def test_restatement_is_pcg_against_scipy(name, tmp, golden):
    """test_sgs_host.py's bound: 10 x the recorded value, and the recorded value is rounding (< 1e-14)"""
    pytest.importorskip("scipy")
    c = mg_cases.SCIPY_CASES[name]
    gap, true_res, eps, k = scipy_gap(c, tmp)
    rec = golden["scipy_gap"][name]
    print("scipy_gap", name, gap, "recorded", rec, "k", k, "true residual / eps", true_res / eps)
    assert 0.0 < rec < 1e-14
    assert gap <= 10.0 * rec
    assert k < c["itermax"]
    assert true_res <= 10.0 * eps


def test_geometric_rule_and_injection_map_are_the_host_librarys():
    from sparsebench_amd import hostapi
    for dims, auto in (((16, 16, 16), 4), ((4, 4, 4), 2), ((12, 8, 20), 3), ((34, 6, 10), 2), ((5, 8, 8), 1), ((2, 2, 2), 1),
                       ((128, 128, 128), 4), ((64, 32, 24), 4), ((8, 8, 4), 2)):
        assert ref.geometric_levels(dims) == hostapi.mg_levels(*dims) == auto, dims
        for L in range(1, auto + 1):
            assert ref.geometric_levels(dims, L) == hostapi.mg_levels(*dims, levels=L) == L
        if auto > 1:
            f2c = ref.geometric_f2c(dims)
            assert np.array_equal(hostapi.mg_f2c(*dims), f2c) and len(np.unique(f2c)) == len(f2c) == np.prod(dims) // 8
            nx, ny, nz = dims
            x, y, z = f2c % nx, f2c // nx % ny, f2c // (nx * ny)
            assert not (x % 2).any() and not (y % 2).any() and not (z % 2).any()
            assert np.array_equal((z // 2 * (ny // 2) + y // 2) * (nx // 2) + x // 2, np.arange(len(f2c)))
    # refusals, each saying which rule failed: an odd dimension, too deep for the divisibility, a coarse dimension below 2
    for dims, L, msg in (((5, 8, 8), 2, "divisible by 2"), ((12, 8, 20), 4, "divisible by 8"), ((16, 16, 16), 5, "coarse dimension smaller than 2"),
                         ((2, 2, 2), 2, "coarse dimension smaller than 2"), ((16, 16, 16), 6, "divisible by 32")):
        with pytest.raises(ValueError, match=msg):
            hostapi.mg_levels(*dims, levels=L)
        with pytest.raises(ValueError, match=msg):
            ref.geometric_levels(dims, L)
    with pytest.raises(ValueError, match="1 or more"):
        hostapi.mg_levels(8, 8, 8, levels=0)
    with pytest.raises(ValueError, match="odd dimension"):
        hostapi.mg_f2c(5, 8, 8)


def counts(c, tmp):
    hier, f2cs, op, b, dinv, eps = ref.build_case(ref.MG, c, tmp)
    out = dict(k_jacobi=pcg_ref.solve(op, b, dinv, c["itermax"], eps)["k"],
               k_sgs=ref.solve(op, ref.sgs(hier.lev[0].g, op), b, dinv, c["itermax"], eps)["k"],
               k_two_sweeps=ref.solve(op, ref.TwoSweeps(hier.lev[0]), b, dinv, c["itermax"], eps)["k"],
               k_mg=ref.solve(op, hier, b, dinv, c["itermax"], eps)["k"], L=hier.L)
    hier.free()
    return out


@pytest.mark.parametrize("name", list(mg_cases.COUNT_CASES))
def test_iteration_count_drops_against_sgs_and_jacobi(name, tmp, golden):
    """MG < SGS < Jacobi -- and the count beside it that says where the drop comes from: the two sweeps of level 0 without any
    coarse level reach eps in as many iterations as the whole cycle (test_what_the_coarse_levels_add)"""
    c = mg_cases.COUNT_CASES[name]
    k = counts(c, tmp)
    print(name, k)
    assert k["k_mg"] < k["k_sgs"] < k["k_jacobi"] < c["itermax"]
    assert golden["counts"][name] == k


def hierarchy_effect(hier, seed=1):
    """||rc|| / ||r|| on level 0 after the pre-smoothing, and V(0, r) against the two sweeps without coarse levels"""
    r = np.random.RandomState(seed).standard_normal(hier.n)
    V = hier.lev[0]
    z0 = V.smoother.pre(r)[0]
    rc = V.transfer.restrict(V, r, z0)
    z, two = hier.apply(r)[0], ref.TwoSweeps(V).apply(r)[0]
    return float(np.linalg.norm(rc) / np.linalg.norm(r)), z, two


@pytest.mark.parametrize("which", ["hpcg16_crs_L4", "hpcg16_sell_64_1_L4", "hand_made_crs"])
def test_in_the_natural_order_the_coarse_levels_are_idle(which, tmp):
    """What the contract's injection and colouring do together.  In the natural row order (CRS, Sell with sigma = 1) the greedy
    colouring of the stencil on an even grid is the parity colouring, and the coarse points (2x, 2y, 2z) are exactly colour 0 (the
    even rows of the tridiagonal matrix likewise).  Colour 0 is the last the pre-smoothing's backward sweep solves, so the residual
    there is rounding; and it is the first the post-smoothing's forward sweep recomputes from the other colours' z, so whatever the
    prolongation added is overwritten.  The cycle is then the two sweeps of level 0 BIT FOR BIT, whatever the coarse levels hold."""
    c = {"hpcg16_crs_L4": dict(matrix=("hpcg", 16), fmt="crs", C=64, sigma=1, levels=4),
         "hpcg16_sell_64_1_L4": dict(matrix=("hpcg", 16), fmt="scs", C=64, sigma=1, levels=4), "hand_made_crs": hand_made_case(tmp)}[which]
    hier, f2cs = ref.build_hierarchy(ref.MG, c, tmp)
    V = hier.lev[0]
    fine = V.transfer.fine
    assert set(V.smoother.colour[fine].tolist()) == {0} and len(fine) == len(V.smoother.rows[0])  # coarse points == colour 0
    rel, z, two = hierarchy_effect(hier)
    print(which, "||rc|| / ||r||", rel)
    assert rel <= 64 * EPS
    assert bits_equal(z, two)
    hier.free()


@pytest.mark.parametrize("which", ["hpcg16_sell_64_256_L4", "hand_made_permuted"])
def test_in_a_permuted_order_the_coarse_levels_change_the_cycle(which, tmp):
    """with sigma > 1 the rows are sorted by length before they are coloured, the parity classes take their colours in another
    sequence and the coarse points are no longer colour 0: the restricted residual is a real one and the cycle is no longer the
    two sweeps (the tests that compare the GPU's restriction and prolongation with the restatement stand on these orders)"""
    c = {"hpcg16_sell_64_256_L4": dict(matrix=("hpcg", 16), fmt="scs", C=64, sigma=256, levels=4),
         "hand_made_permuted": hand_made_case(tmp, "scs", 256)}[which]
    hier, f2cs = ref.build_hierarchy(ref.MG, c, tmp)
    V = hier.lev[0]
    assert 0 not in set(V.smoother.colour[V.transfer.fine].tolist())
    rel, z, two = hierarchy_effect(hier)
    diff = float(np.linalg.norm(z - two) / np.linalg.norm(z))
    print(which, "||rc|| / ||r||", rel, "||V(r) - two sweeps|| / ||V(r)||", diff)
    assert rel > 1e-3 and diff > 1e-4
    hier.free()


def golden_record(out):
    rec = pcg_ref.record(out)
    rec["nC"], rec["L"], rec["rows"] = [int(v) for v in out["nC"]], int(out["L"]), [int(v) for v in out["rows"]]
    return rec


@pytest.mark.parametrize("name", mg_cases.SMALL)
def test_the_committed_golden_is_what_the_restatement_gives(name, tmp, golden):
    assert golden_record(ref.run_case(ref.MG, mg_cases.CASES[name], tmp)) == golden["cases"][name]
    assert set(golden["cases"]) == set(mg_cases.CASES)
