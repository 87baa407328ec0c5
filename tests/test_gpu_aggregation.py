"""The smoothed-aggregation prolongation on the GPU == its CPU restatement (tests/aggregation_ref.py, pinned by
tests/test_aggregation_ref.py) BIT FOR BIT: agg, n_agg, rounds, and the pointers, columns and values of P -- on generated grids in
CRS, Sell-64-1, Sell-64-256 and Sell-4-8 (a real permutation), identical across the formats, and on hand-made matrices through
Problem.from_csr; the hierarchy; the whole solves of tests/aggregation_cases.py under PCG and BiCGStab in both kernel modes against
tests/golden/aggregation_hist.json (k, every history, x); coarsening="geometric" is the handle of before; the refusals, each in a
child process.

No launch of aggregation.hip.h is capped or grid-strided (a thread per row, the grid covers every row), so there is no launch
query and no capped-launch case.

The values of the NaN matrix are compared bit for bit where they are numbers and by position where they are NaN: IEEE 754 leaves
the sign and payload a NaN takes through an operation to the implementation, and t - u is a subtraction on the host and may be an
addition of a negated operand on the device."""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import aggregation_cases as ac
import aggregation_ref as ar
import galerkin_ref as gr
import pcg_ref
from conftest import load_json
from sparsebench_amd import hostapi
from test_gpu_mg import collect, modes, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return load_json("aggregation_hist.json")


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("aggregation_gpu")


@functools.lru_cache(maxsize=None)
def grid_ref(dims):
    """the restatement on a grid, computed once for the four formats: (aggregate's triple, prolongation's, the tentative T)"""
    A = gr.stencil(dims)
    return ar.aggregate(A), ar.prolongation(A), ar.prolongation(A, omega_s=0.0)


def stored(p):
    """the matrix as the device stores its rows"""
    return (p.array("rowPtr").astype(np.uint64),) + tuple(p.gm_entries())


def check_aggregate(p, theta, want, what):
    agg, n_agg, rounds = hostapi.aggregate(p, theta)
    assert agg.dtype == np.int32 and np.array_equal(agg, want[0]), (what, "agg", np.nonzero(agg != want[0])[0][:8])
    assert (n_agg, rounds) == (want[1], want[2]), (what, n_agg, rounds, want[1:3])


@pytest.mark.parametrize("fname", list(ar.FORMATS))
@pytest.mark.parametrize("dims", ar.GRIDS, ids=lambda d: "%dx%dx%d" % d)
def test_generated_grids_equal_the_restatement_in_every_format(gpu, dims, fname, golden):
    fmt = ar.FORMATS[fname]
    p = hostapi.Problem("generate", *dims, fmt=fmt[0], Cc=fmt[1], sigma=fmt[2])
    if fname == "sell_4_8" and p.nr > 8:
        assert not np.array_equal(p.array("oldToNewPerm"), np.arange(p.nr)) or dims == (2, 2, 2)
    want_agg, want_p, want_t = grid_ref(dims)
    check_aggregate(p, 0.0, want_agg, (dims, fname))
    P, n_agg, st = hostapi.sa_prolongation(p, stats=True)
    gr.same_csr(P, want_p[0], (dims, fname, "P"))
    assert n_agg == want_p[1] and st["rounds"] == want_p[2]
    T, n_t = hostapi.sa_prolongation(p, omega_s=0.0)
    gr.same_csr(T, want_t[0], (dims, fname, "T"))
    assert n_t == n_agg and set(T[2].tolist()) == {1.0} and len(T[1]) == p.nr
    e = golden["prolongations"]["dims_%d_%d_%d" % dims]
    assert gr.digest(P) == {"nnz": e["nnz"], "sha256": e["sha256"]} and (n_agg, st["rounds"]) == (e["n_agg"], e["rounds"])
    if dims == (2, 2, 2):
        assert n_agg == 1 and set(want_agg[0].tolist()) == {0}  # every row sees every row
    p.free()


@pytest.mark.parametrize("fname", ["crs", "sell_4_8"])
@pytest.mark.parametrize("name", list(ar.HAND_MADE))
def test_hand_made_matrices_equal_the_restatement(gpu, name, fname, golden):
    A, theta = ar.HAND_MADE[name]()
    fmt = ar.FORMATS[fname]
    p = hostapi.Problem.from_csr(*A, fmt=fmt[0], Cc=fmt[1], sigma=fmt[2])
    S = stored(p)
    assert np.array_equal(S[0], A[0]) and np.array_equal(S[1], A[1])  # ascending columns: stored as given
    want = ar.aggregate(S, theta)
    check_aggregate(p, theta, want, (name, fname))
    P, n_agg = hostapi.sa_prolongation(p, theta, lmax=ac.HAND_LMAX)
    wantP = ar.prolongation(S, theta, lmax=ac.HAND_LMAX)[0]
    if name == "nan":
        gr.same_csr(P[:2] + (np.zeros(0),), wantP[:2] + (np.zeros(0),), (name, fname))
        nan = np.isnan(wantP[2])
        assert nan.any() and np.array_equal(np.isnan(P[2]), nan)
        assert np.array_equal(P[2][~nan].view(np.uint64), wantP[2][~nan].view(np.uint64))
    else:
        gr.same_csr(P, wantP, (name, fname))
        e = golden["prolongations"][name]
        assert gr.digest(P) == {"nnz": e["nnz"], "sha256": e["sha256"]} and n_agg == e["n_agg"]
    if name == "threshold":
        assert want[0].tolist()[5:] == [-1, -1] and want[1] == 1  # the entry at the threshold and the stored 0.0 are not strong
    if name == "one_way":
        assert want[0][4] >= 0 and want[0][5] >= 0  # reached along their own out-edges only
    p.free()


@pytest.mark.parametrize("fname", ["crs", "sell_64_256", "sell_4_8"])
def test_scaled_matrix_whose_products_are_not_exact(gpu, fname):
    fmt = ar.FORMATS[fname]
    p = hostapi.Problem.from_csr(*gr.scaled_hpcg8(), fmt=fmt[0], Cc=fmt[1], sigma=fmt[2])
    S = stored(p)
    # theta = 1 / 27 is the ratio |a| / sqrt(d_i d_j) of EVERY off-diagonal entry in exact arithmetic: rounding decides which 8108
    # of the 10136 are strong, and the graph is no longer symmetric
    assert len(ar.strong_graph(S, 1.0 / 27.0)[1]) == 8108
    for theta, omega_s in ((0.0, 4.0 / 3.0), (1.0 / 27.0, 1.0)):
        check_aggregate(p, theta, ar.aggregate(S, theta), ("scaled8", fname, theta))
        P, n_agg = hostapi.sa_prolongation(p, theta, omega_s)
        want = ar.prolongation(S, theta, omega_s)
        gr.same_csr(P, want[0], ("scaled8", fname, theta))
        assert n_agg == want[1]
    p.free()


def test_hierarchy_equals_the_restatements(gpu):
    dims = (12, 8, 20)
    mats, steps = ar.hierarchy(gr.stencil(dims))
    assert len(mats) >= 2
    p = hostapi.Problem("generate", *dims, fmt="scs", Cc=64, sigma=256)
    found = hostapi.mg_aggregation(p)
    assert len(found) == len(mats) - 1
    for (q, P, omega), M, (wantP, n_agg, rounds) in zip(found, mats[1:], steps):
        assert omega == 1.0 and q.filename == "memory" and (q.fmt, q.Cc, q.sigma_arg) == ("scs", 64, 256)
        gr.same_csr(P, wantP, "P")
        gr.same_csr(stored(q), M, "A_c")
        assert q.nr == n_agg and q.aggregation_stats["rounds"] == rounds
    for q, _, _ in found:
        q.free()
    p.free()


def test_a_level_that_coarsens_by_less_than_two_is_refused_by_name(gpu):
    """130 rows that each point at row 0 alone, which points at nothing: every one of them is its own root"""
    A, theta = ar.arrow(130)
    agg, n_agg, rounds = ar.aggregate(A, theta)
    assert n_agg == 129 and agg[0] == -1
    p = hostapi.Problem.from_csr(*A, fmt="crs")
    check_aggregate(p, theta, (agg, n_agg, rounds), "arrow")
    with pytest.raises(ValueError, match="level 0: 129 aggregates of 130 rows: the level coarsens by less than 2"):
        hostapi.mg_aggregation(p)
    with pytest.raises(ValueError, match="coarsens by less than 2"):
        hostapi.PCG(p, precond="mgpoly", coarsening="aggregation")
    p.free()


def check_golden(got, rec, keys, what):
    want = {key: pcg_ref.unhex(rec[key]) for key in keys}
    want["k"] = rec["k"]
    same(got, want, what, keys=keys)
    assert hashlib.sha256(np.ascontiguousarray(got["x"], dtype=np.float64).tobytes()).hexdigest() == rec["x_sha256"], (what, "x")


@pytest.mark.parametrize("name", list(ac.SOLVES))
def test_whole_solves_equal_the_restatements_golden(gpu, name, golden, tmp):
    c, rec = ac.SOLVES[name], golden["solves"][name]
    eps = float.fromhex(rec["eps"])
    p = ac.problem(c["matrix"], c["fmt"], tmp)
    seen = modes(p)
    if c["matrix"][0] == "hpcg" and c["fmt"][0] == "scs":
        assert seen == [5, 0], seen  # the generated stencil in Sell-64 has row programs: both kernels run
    for mode in seen:
        assert p.use_packed(mode) == mode
        if c["solver"] == "pcg":
            s = hostapi.PCG(p, precond="mgpoly", coarsening="aggregation", steps=c["steps"])
            M = s
            got, keys = collect(s, s.solve(ac.ITERMAX, eps)), ("rr", "rz", "pAp")
        else:
            s = hostapi.BiCGStab(p, precond="mgpoly", coarsening="aggregation", steps=c["steps"])
            M = s.pcg
            assert s.precond() == "mgpoly" and s.launches_per_body() == rec["launches"]
            k = s.solve(ac.ITERMAX, eps)
            got, keys = dict(s.history(), k=k, x=s.solution()), ("rr", "rho", "rv", "ts", "tt")
        assert [M.level_rows(l) for l in range(M.levels())] == rec["rows"], (name, mode)
        assert [q.aggregation_stats["rounds"] for q in M._owned] == rec["rounds"]
        check_golden(got, rec, keys, (name, mode))
        assert 1 < got["k"] < ac.ITERMAX
        owned = list(M._owned)
        s.free()
        assert all(q.ptr is None for q in owned)  # the coarse problems went with the handle
    p.free()


def test_geometric_coarsening_is_the_handle_of_before(gpu):
    p = hostapi.Problem("generate", 16, 16, 16, fmt="scs", Cc=64, sigma=256)
    runs = []
    for kw in (dict(levels=3), dict(levels=3, galerkin="device")):
        for extra in ({}, dict(coarsening="geometric")):
            s = hostapi.PCG(p, precond="mgpoly", **kw, **extra)
            runs.append(collect(s, s.solve(150, 1e-8)))
            s.free()
        same(runs[-1], runs[-2], kw)
    e = load_json("mg_poly_hist.json")["cases"]["hpcg16_sell_64_256_L3"]
    s = hostapi.PCG(p, precond="mgpoly", levels=3, coarsening="geometric")
    from test_gpu_mg import same_as_golden
    same_as_golden(collect(s, s.solve(150, float.fromhex(e["eps"]))), e, "geometric")
    s.free()
    for bad in (dict(precond="mgpoly", coarsening="aggregation", galerkin=True), dict(precond="poly", coarsening="aggregation"),
                dict(precond="mgpoly", theta=0.1), dict(precond="mgpoly", coarsening="other")):
        with pytest.raises(ValueError):
            hostapi.PCG(p, **bad)
    p.free()


CHILD = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
what = sys.argv[1]
from sparsebench_amd import capi, hostapi
import numpy as np
import ctypes as C
import aggregation_ref as ar
L = capi.init(0)
n_agg, rounds = C.c_uint32(0), C.c_uint32(0)
if what == "sp":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1, precision="single")
    L.sb_matrix_aggregate(p.matrix, 0.0, None, C.byref(n_agg), C.byref(rounds))
elif what == "zero_diagonal":
    (ptr, col, val), _ = ar.chain(10)
    val[int(ptr[4]) + 1] = 0.0
    p = hostapi.Problem.from_csr(ptr, col, val, fmt="crs")
    L.sb_matrix_aggregate(p.matrix, 0.0, None, C.byref(n_agg), C.byref(rounds))
elif what == "theta":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=256)
    L.sb_matrix_sa_prolongation(p.matrix, -0.25, 1.0, 0.0, C.byref(n_agg))
elif what == "isolated":
    p = hostapi.Problem.from_csr(*ar.all_isolated(5)[0], fmt="crs")
    L.sb_matrix_aggregate(p.matrix, 0.0, None, C.byref(n_agg), C.byref(rounds))
    assert (n_agg.value, rounds.value) == (0, 0)
    print("AGGREGATE GAVE NONE")
    L.sb_matrix_sa_prolongation(p.matrix, 0.0, 1.0, 0.0, C.byref(n_agg))
print("NOT REFUSED")
"""

REFUSALS = [("sp", "sb_matrix_aggregate: double precision only (the matrix was uploaded in single precision)"),
            ("zero_diagonal", "sb_matrix_aggregate: 1 of 10 matrix rows have a diagonal entry that is zero or not finite (the first: device row 4)"),
            ("theta", "sb_matrix_sa_prolongation: theta = -0.25: the strength threshold must be finite and not negative"),
            ("isolated", "sb_matrix_sa_prolongation: no root: every one of the 5 rows is isolated")]


@pytest.mark.parametrize("what,msg", REFUSALS)
def test_refusals_end_the_process_with_their_message(gpu, what, msg):
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), what], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    err, txt = out.stderr.decode(), out.stdout.decode()
    assert out.returncode == 1, (out.returncode, err[-1000:])
    assert msg in err and "sbhip:" in err and "NOT REFUSED" not in txt, err[-1000:]
    assert (what != "isolated") or "AGGREGATE GAVE NONE" in txt
    assert "illegal memory access" not in err and "HIP error" not in err
