"""PCG with the Chebyshev-smoothed V-cycle on the GPU == the CPU restatement of its contract (tests/precond_ref.py,
pinned by tests/test_mg_poly_host.py) and tests/golden/mg_poly_hist.json BIT FOR BIT: k, every r.r, every r.z, every p.Ap, x and
dinv, in both kernel modes of the SpMV, on the regenerated hierarchy, on a caller's and on the Galerkin one.  Without coarse
levels the solver is hostapi.PCG(precond="poly") bit for bit; a solve in pieces and a second solve repeat the first; the other
kinds of handle on the same problem give their own goldens before and after; every refusal of sb_pcg_create_mg_poly ends the
process with its message.  (NaN compares equal to NaN.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import mg_fw_cases
import mg_poly_cases as cases
import pcg_cases
import pcg_ref
import poly_cases
import precond_ref as ref
from conftest import load_json
from sparsebench_amd import hostapi
from test_gpu_mg import collect, check_counters, same, same_as_golden, modes, files

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("mg_poly_gpu")


@pytest.fixture(scope="module")
def golden():
    return load_json("mg_poly_hist.json")


def steps_of(c):
    return {k: c[k] for k in ("steps", "coarse_steps", "lmax", "ratio") if c.get(k) is not None}


def handle(c, tmp):
    """(problem, the coarse problems the caller owns, a constructor of handles) of a case"""
    p = hostapi.Problem(*pcg_ref.problem_args(c["matrix"], tmp), fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])
    if c.get("coarse") is None:
        return p, [], lambda: hostapi.PCG(p, precond="mgpoly", levels=c.get("levels"), galerkin=bool(c.get("galerkin")), **steps_of(c))
    coarse = []
    for (matrix, _, _), (P, omega) in zip(c["coarse"], ref.case_transfers(ref.MGPOLY, c)):
        q = hostapi.Problem(*pcg_ref.problem_args(matrix, tmp), fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])
        coarse.append((q, P, omega))
    return p, [q for q, _, _ in coarse], lambda: hostapi.PCG(p, precond="mgpoly", coarse=coarse, **steps_of(c))


@pytest.mark.parametrize("name", cases.SMALL)
def test_gpu_equals_the_restatement_and_the_golden(gpu, name, tmp, golden):
    c = cases.CASES[name]
    hier, transfers, op, b, dinv, eps = ref.build_case(ref.MGPOLY, c, tmp)
    want = ref.solve(op, hier, b, dinv, c["itermax"], eps)
    want["dinv"] = op.to_orig(hier.dinv)
    e = golden["cases"][name]
    assert eps == float.fromhex(e["eps"]) and e["L"] == hier.L
    p, owned, make = handle(c, tmp)
    assert np.array_equal(p.rhs()[0], b)
    seen = modes(p)
    if name.startswith("hpcg"):
        assert seen == [5, 0], seen
    for mode in seen:
        assert p.use_packed(mode) == mode
        s = make()
        assert s.precond() == "mgpoly" and s.levels() == hier.L and s.colours() == 0
        assert [s.level_rows(l) for l in range(hier.L)] == e["rows"]
        for l in range(hier.L):
            assert [float(v).hex() for v in s.coeffs(l)] == e["coeffs"][l], (name, l)
            assert [float(v).hex() for v in s.interval(l)] == e["intervals"][l], (name, l)
        fused = c["fmt"] == "scs" or mode == 5
        assert s.launches_per_body() == e["launches"] + (0 if fused else 1) and s.precond_bytes() == e["bytes"]
        got = collect(s, s.solve(c["itermax"], eps))
        check_counters(s, got)  # the device's own counters: bodies run, history entries written
        same(got, want, (name, mode))
        same_as_golden(got, e, (name, mode))
        if mode == seen[0]:  # a second solve on the handle repeats the first
            same(collect(s, s.solve(c["itermax"], eps)), got, (name, "again"))
        if c.get("galerkin"):  # the handle owns the coarse problems and their files, and takes them with it
            d = s._owned_dir
            assert len(s._owned) == hier.L - 1 and sorted(os.listdir(d)) == ["level%d.mtx" % l for l in range(1, hier.L)]
            s.free()
            assert not os.path.exists(d) and s._owned == []
        else:
            s.free()
    assert 1 < want["k"] < c["itermax"]  # eps was reached in the middle
    for q in owned:
        q.free()
    p.free(), hier.free()


def test_galerkin_coarse_operators_through_the_callers_door(gpu, tmp):
    """mg_galerkin's list handed in as coarse= is galerkin=True bit for bit, and fewer iterations than the regenerated hierarchy"""
    p = hostapi.Problem("generate", 16, 16, 16, fmt="scs", Cc=64, sigma=256)
    b = p.rhs()[0]
    eps = 1e-10 * float(np.sqrt(b @ b))
    own = hostapi.PCG(p, precond="mgpoly", levels=3, galerkin=True)
    want = collect(own, own.solve(150, eps))
    d = tmp / "galerkin_door"
    d.mkdir()
    coarse = hostapi.mg_galerkin(p, levels=3, directory=d)
    s = hostapi.PCG(p, precond="mgpoly", coarse=coarse)
    same(collect(s, s.solve(150, eps)), want, "coarse=mg_galerkin(...) == galerkin=True")
    reg = hostapi.PCG(p, precond="mgpoly", levels=3)
    assert want["k"] < reg.solve(150, eps)
    reg.free(), s.free(), own.free()
    assert sorted(os.listdir(d)) == ["level1.mtx", "level2.mtx"]  # the caller's files stay
    for q, _, _ in coarse:
        q.free()
    p.free()


def test_no_coarse_level_is_poly_pcg_solves_repeat_and_other_kinds_are_untouched(gpu, tmp):
    c = poly_cases.CASES["scaled16_sell_64_256_eps"]
    p = hostapi.Problem(*pcg_ref.problem_args(c["matrix"], tmp), fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])
    b = p.rhs()[0]
    eps = 1e-10 * float(np.sqrt(b @ b))
    # the other kinds of handle on this problem, before anything of the new kind exists
    kinds = dict(jacobi={}, poly=dict(precond="poly"), sgs=dict(precond="sgs"))
    before = {}
    for kind, kw in kinds.items():
        h = hostapi.PCG(p, **kw)
        before[kind] = collect(h, h.solve(150, eps))
        h.free()
    for cs in (1, 3):
        q = hostapi.PCG(p, precond="poly", steps=cs)
        want = collect(q, q.solve(150, eps))
        one = hostapi.PCG(p, precond="mgpoly", coarse=[], steps=5, coarse_steps=cs, ratio=16.0)
        assert one.levels() == 1 and one.precond() == "mgpoly" and one.level_steps(0) == cs and 1 < want["k"] < 150
        assert one.launches_per_body() == q.launches_per_body() and one.precond_bytes() == q.precond_bytes()
        same(collect(one, one.solve(150, eps)), want, "no coarse level == the polynomial handle")
        r = ref.probe_vector(p.nr, 3, True)
        assert pcg_ref.same_bits(one.apply(r), q.apply(r))
        one.free(), q.free()
    # two levels: in uneven pieces, then another itermax, an apply and a probe in between, then the first again
    coarse = hostapi.Problem("generate", 8, 8, 8, fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])
    two = hostapi.PCG(p, precond="mgpoly", coarse=[(coarse, hostapi.mg_trilinear(16, 16, 16), 0.5)])
    first = collect(two, two.solve(150, eps))
    assert 1 < first["k"] < 150
    two.start(150, eps)
    for n in (1, 4, 2, 7, 3, 11, 5, 13):
        two.run_iters(n)
    same(collect(two, two.finish()), first, "pieces")
    short = collect(two, two.solve(7, 0.0))
    assert short["k"] == 7
    for key in ("rr", "rz", "pAp"):
        assert pcg_ref.same_bits(short[key][:6], first[key][:6]), key
    z = two.apply(b)
    two.mg_poly_probe(0, b, z, z, np.ones(512))
    same(collect(two, two.solve(150, eps)), first, "after another solve, an apply and a probe")
    assert np.isfinite(z).all() and two.loop_ms() > 0.0
    for kind, kw in kinds.items():  # ... and after
        h = hostapi.PCG(p, **kw)
        same(collect(h, h.solve(150, eps)), before[kind], kind + " after mgpoly")
        h.free()
    two.free(), coarse.free(), p.free()


def test_jacobi_mgfw_and_poly_handles_still_give_their_goldens(gpu, tmp):
    """one case each of the neighbours' committed goldens, with an mgpoly handle alive on the same problem"""
    c = mg_fw_cases.CASES["hpcg16_sell_64_256_L3"]
    p = hostapi.Problem("generate", 16, 16, 16, fmt="scs", Cc=64, sigma=256)
    alive = hostapi.PCG(p, precond="mgpoly", levels=3)
    alive.solve(20, 0.0)
    e = load_json("mg_fw_hist.json")["cases"]["hpcg16_sell_64_256_L3"]
    s = hostapi.PCG(p, precond="mgfw", levels=3)
    same_as_golden(collect(s, s.solve(c["itermax"], float.fromhex(e["eps"]))), e, "mgfw")
    s.free()
    for kind, file, name in (("poly", "poly_hist.json", "hpcg16_sell_64_256_eps"), ("jacobi", "pcg_hist.json", "hpcg16_sell_64_256")):
        e = load_json(file)["cases"][name]
        src = (poly_cases.CASES if kind == "poly" else pcg_cases.CASES)[name]
        assert (src["matrix"], src["fmt"], src["C"], src["sigma"]) == (("hpcg", 16), "scs", 64, 256) and src.get("dinv", "jacobi") == "jacobi"
        s = hostapi.PCG(p, precond=kind)
        same_as_golden(collect(s, s.solve(src["itermax"], float.fromhex(e["eps"]))), e, kind)
        s.free()
    alive.free(), p.free()


def test_check_residual_and_exact_solution(gpu):
    p = hostapi.Problem("generate", 16, 16, 16, fmt="scs", Cc=64, sigma=256)
    s = hostapi.PCG(p, precond="mgpoly")
    assert s.levels() == 4 and s.steps() == 2 and s.level_steps(3) == 2  # auto: HPCG's depth, the default steps
    k = s.solve(150, 1e-9)
    assert 1 < k < 150
    x = s.solution()
    assert s.check_residual() == np.max(np.abs(x - 1.0)) < 1e-8
    s.free(), p.free()


CHILD = r"""
import sys
sys.path.insert(0, %r)
what = sys.argv[1]
from sparsebench_amd import capi, hostapi
import numpy as np
L = capi.init(0)
p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
ptr, col, val = hostapi.mg_trilinear(8, 8, 8)
omega, kw = 0.25, {}
if what == "sp":
    q = hostapi.Problem("generate", 4, 4, 4, fmt="scs", Cc=64, sigma=1, precision="single")
    q.precision = "double"  # past hostapi's own refusal: the library's is the one under test
elif what == "not_smaller":
    q = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1)
else:
    q = hostapi.Problem(sys.argv[3] if what == "zero_diagonal" else "generate", 4, 4, 4, fmt="scs", Cc=64, sigma=1)
    col = np.minimum(col, q.nr - 1)
if what == "column":
    col[100] = 64
if what == "pointer":
    ptr[201] = ptr[200] - 1
if what == "weight_nan":
    val[33] = np.nan
if what == "omega_zero":
    omega = 0.0
    hostapi._omega = lambda omega, l: omega  # past hostapi's own refusal
if what in ("steps", "coarse_steps", "ratio", "lmax"):
    hostapi.PCG._poly_args = staticmethod(lambda steps, lmax, ratio, what="steps": (steps, 0.0 if lmax is None else lmax, ratio))
    kw = dict(steps=dict(steps=17), coarse_steps=dict(coarse_steps=-1), ratio=dict(ratio=1.0), lmax=dict(lmax=float("inf")))[what]
if what == "seq":
    L.sb_set_dot_order(1)
if what == "fine_zero_diagonal":
    p = hostapi.Problem(sys.argv[3], 1, 1, 1, fmt="crs")
    q = hostapi.Problem(sys.argv[4], 1, 1, 1, fmt="crs")
    ptr, col, val = np.arange(7, dtype=np.uint64), np.array([0, 0, 1, 1, 2, 2], np.uint32), np.ones(6)
s = hostapi.PCG(p, precond="mgpoly", coarse=[(q, (ptr, col, val), omega)], **kw)
if what == "probe_in_flight":
    s.start(10, 0.0)
    s.mg_poly_probe(0, np.ones(512), np.ones(512), np.ones(512), np.ones(64))
if what == "probe_last_level":  # (hostapi's own refusal passed by: the library's is the one under test)
    v = [hostapi._ptr(np.ones(64)) for _ in range(6)]
    L.sb_pcg_mg_poly_probe(s.ptr, 1, *v)
print("NOT REFUSED")
"""

REFUSALS = [("sp", "sb_pcg_create_mg_poly: MG: double precision only (the matrix of level 1"),
            ("not_smaller", "sb_pcg_create_mg_poly: level 1 has 512 rows, level 0 has 512: every level must be smaller"),
            ("column", "sb_pcg_create_mg_poly: level 0: the prolongation's row"),
            ("column", "has column 64 outside the 64 rows of level 1"),
            ("pointer", "sb_pcg_create_mg_poly: level 0: the prolongation's row pointer falls from"),
            ("weight_nan", "has a weight that is not finite"),
            ("omega_zero", "sb_pcg_create_mg_poly: omega[0] = 0: the restriction's scale of level 0 must be finite and positive"),
            ("steps", "sb_pcg_create_mg_poly: steps = 17: the smoother has 1 to 16 steps"),
            ("coarse_steps", "sb_pcg_create_mg_poly: coarse_steps = -1: the coarsest level's polynomial has 1 to 16 steps"),
            ("ratio", "sb_pcg_create_mg_poly: ratio = 1: lmax / lmin must be finite and greater than 1"),
            ("lmax", "sb_pcg_create_mg_poly: lmax = inf: the caller's lmax must be finite"),
            ("zero_diagonal", "2 of 6 matrix rows have no finite positive diagonal entry (the first: device row 2): the MG-Chebyshev (level 1) preconditioner"),
            ("fine_zero_diagonal", "2 of 6 matrix rows have no finite positive diagonal entry (the first: device row 2): the MG-Chebyshev (level 0) preconditioner"),
            ("probe_in_flight", "sb_pcg_mg_poly_probe between sb_pcg_start and sb_pcg_finish"),
            ("probe_last_level", "sb_pcg_mg_poly_probe: level 1 of a handle with 2 levels has no transfers"),
            ("seq", "tree dot order only")]


@pytest.mark.parametrize("what,msg", REFUSALS)
def test_refusals_end_the_process_with_their_message(gpu, what, msg, tmp):
    """host-side checks and the diagonal count: fatal with file:line, exit status 1, no GPU fault"""
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT, what] + list(files(tmp)), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    err = out.stderr.decode()
    assert out.returncode == 1, (out.returncode, err[-1000:])
    assert msg in err and "sbhip:" in err and "NOT REFUSED" not in out.stdout.decode(), err[-1000:]
    assert "illegal memory access" not in err and "HIP error" not in err


@pytest.mark.parametrize("name", [n for n in cases.CASES if cases.CASES[n].get("big")])
def test_big_case_against_the_committed_golden(gpu, name, golden):
    """HPCG 32^3 at HPCG's depth: tests/golden/mg_poly_hist.json, made by the CPU restatement"""
    c = cases.CASES[name]
    e = golden["cases"][name]
    p = hostapi.Problem(*pcg_ref.problem_args(c["matrix"]), fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])
    for mode in modes(p):
        p.use_packed(mode)
        s = hostapi.PCG(p, precond="mgpoly", levels=c["levels"])
        assert [s.level_rows(l) for l in range(s.levels())] == e["rows"] and s.launches_per_body() == e["launches"] == 37
        got = collect(s, s.solve(c["itermax"], float.fromhex(e["eps"])))
        s.free()
        same_as_golden(got, e, (name, mode))
        assert 1 < got["k"] < c["itermax"]
    p.free()
