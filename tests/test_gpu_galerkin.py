"""The device Galerkin hierarchy on the GPU: mg_galerkin(product="device") gives the scipy path's problems bit for
bit at HPCG 16^3; PCG(galerkin="device") == PCG(galerkin=True) in k, r.r, r.z, p.Ap, x, per-level intervals and coefficients,
launches per body and precond_bytes for the committed Galerkin cases of tests/golden/mg_poly_hist.json (and therefore equal to that
golden) at 1 and 2 steps; on the scaled 8^3 matrix, whose products are not exact, the two-level solve on the device's operator is
the CPU restatement (precond_ref.Hierarchy over galerkin_ref's operator) and tests/golden/galerkin_hist.json bit for bit; the
other kinds of handle give their own goldens before and after; freeing the handle frees the coarse problems and no directory is
made; the library's refusals end a child process with their message."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import galerkin_ref as gr
import mg_fw_cases
import mg_poly_cases as cases
import pcg_cases
import pcg_ref
import poly_cases
import precond_ref as ref
from conftest import load_json
from sparsebench_amd import hostapi
from test_gpu_mg import collect, same, same_as_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("fmt,C,sigma", [("crs", 64, 1), ("scs", 64, 256)])
def test_device_hierarchy_is_the_scipy_paths_bit_for_bit(gpu, fmt, C, sigma, tmp_path):
    pytest.importorskip("scipy")
    p = hostapi.Problem("generate", 16, 16, 16, fmt=fmt, Cc=C, sigma=sigma)
    before = set(os.listdir(tempfile.gettempdir()))
    dev = hostapi.mg_galerkin(p, levels=3, product="device")
    assert set(os.listdir(tempfile.gettempdir())) == before  # no directory, no files
    host = hostapi.mg_galerkin(p, levels=3, directory=tmp_path)
    assert len(dev) == len(host) == 2 and [q.nr for q, _, _ in dev] == [512, 64]
    for l, ((q, P, omega), (h, Ph, omegah)) in enumerate(zip(dev, host)):
        assert omega == omegah == 1.0 and q.filename == "memory" and (q.fmt, q.Cc, q.sigma_arg) == (fmt, C, sigma)
        assert all(np.array_equal(a, b) for a, b in zip(P, Ph))
        assert np.array_equal(q.array("rowPtr"), h.array("rowPtr")), l
        for a, b in zip(q.gm_entries(), h.gm_entries()):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), l
        assert np.array_equal(q.values().view(np.uint64), h.values().view(np.uint64)), l
        assert q.galerkin_stats["dropped"] == 0 and q.galerkin_stats["max_row_ac"] <= 27
    for q, _, _ in dev + host:
        q.free()
    p.free()


@pytest.mark.parametrize("steps", [1, 2])
@pytest.mark.parametrize("name", ["hpcg16_crs_L3_galerkin", "hpcg16_sell_64_256_L3_galerkin"])
def test_pcg_on_the_device_hierarchy_is_pcg_on_the_scipy_one(gpu, name, steps):
    pytest.importorskip("scipy")
    c = cases.CASES[name]
    assert c["galerkin"] and c["levels"] == 3 and c.get("steps") is None
    e = load_json("mg_poly_hist.json")["cases"][name]
    eps = float.fromhex(e["eps"])
    p = hostapi.Problem(*pcg_ref.problem_args(c["matrix"]), fmt=c["fmt"], Cc=c["C"], sigma=c["sigma"])
    d = hostapi.PCG(p, precond="mgpoly", levels=3, galerkin="device", steps=steps)
    h = hostapi.PCG(p, precond="mgpoly", levels=3, galerkin=True, steps=steps)
    assert d.levels() == h.levels() == 3 and d._owned_dir is None and len(d._owned) == 2
    for l in range(3):
        assert d.level_rows(l) == h.level_rows(l)
        assert [float(v).hex() for v in d.interval(l)] == [float(v).hex() for v in h.interval(l)], (name, l)
        assert pcg_ref.same_bits(d.coeffs(l), h.coeffs(l)), (name, l)
    assert d.launches_per_body() == h.launches_per_body() and d.precond_bytes() == h.precond_bytes()
    got, want = collect(d, d.solve(c["itermax"], eps)), collect(h, h.solve(c["itermax"], eps))
    same(got, want, (name, steps))
    if steps == 2:  # the committed case
        same_as_golden(got, e, name)
        assert [float(v).hex() for v in d.interval(0)] == e["intervals"][0] and d.precond_bytes() == e["bytes"]
    assert 1 < got["k"] < c["itermax"]
    owned = list(d._owned)
    d.free(), h.free()
    assert d._owned == [] and all(q.ptr is None for q in owned)  # the coarse problems went with the handle
    p.free()


@pytest.mark.parametrize("steps", [1, 2])
@pytest.mark.parametrize("fname,fmt", [("crs", ("crs", 64, 1)), ("sell_64_256", ("scs", 64, 256))])
def test_inexact_operator_solve_equals_the_restatement_and_the_golden(gpu, fname, fmt, steps):
    hier, op, b, eps, (A, P, Ac) = gr.scaled_case(fmt, steps)
    dinv = op.to_orig(hier.dinv)
    want = ref.solve(op, hier, b, dinv, 150, eps)
    want["dinv"] = dinv
    e = load_json("galerkin_hist.json")["solves"]["scaled8_%s_steps%d" % (fname, steps)]
    assert eps == float.fromhex(e["eps"])
    p = hostapi.Problem.from_csr(*A, fmt=fmt[0], Cc=fmt[1], sigma=fmt[2])
    assert np.array_equal(p.rhs()[0], b)
    if fmt[2] > 1:  # the restatement walks the device's own permutation
        assert np.array_equal(p.array("oldToNewPerm"), op.o2n if op.o2n is not None else np.arange(p.nr))
    got_ac, st = hostapi.galerkin_product(p, P)
    gr.same_csr(got_ac, Ac, "A_c")
    q = hostapi.Problem.from_csr(*got_ac, fmt=fmt[0], Cc=fmt[1], sigma=fmt[2])
    s = hostapi.PCG(p, precond="mgpoly", coarse=[(q, P, 1.0)], steps=steps)
    got = collect(s, s.solve(150, eps))
    same(got, want, ("scaled 8^3", fname, steps))
    same_as_golden(got, e, ("scaled 8^3", fname, steps))
    assert 1 < got["k"] < 150
    s.free(), q.free(), p.free(), hier.free()


def test_other_kinds_of_handle_still_give_their_goldens_before_and_after(gpu):
    p = hostapi.Problem("generate", 16, 16, 16, fmt="scs", Cc=64, sigma=256)
    import sgs_cases
    runs = []
    for kind, kw, file, name, src in (("mgfw", dict(levels=3), "mg_fw_hist.json", "hpcg16_sell_64_256_L3", mg_fw_cases.CASES),
                                      ("mgpoly", dict(levels=3), "mg_poly_hist.json", "hpcg16_sell_64_256_L3", cases.CASES),
                                      ("poly", {}, "poly_hist.json", "hpcg16_sell_64_256_eps", poly_cases.CASES),
                                      ("jacobi", {}, "pcg_hist.json", "hpcg16_sell_64_256", pcg_cases.CASES),
                                      ("sgs", {}, "sgs_hist.json", "hpcg16_sell_64_256", sgs_cases.CASES)):
        c = src[name]
        assert (c["matrix"], c["fmt"], c["C"], c["sigma"]) == (("hpcg", 16), "scs", 64, 256) and c.get("dinv", "jacobi") == "jacobi"
        assert c.get("levels", 3) == 3 and not c.get("galerkin") and c.get("steps") is None
        runs.append((kind, dict(kw, precond=kind), c["itermax"], load_json(file)["cases"][name]))

    def check(when):
        for kind, kw, itermax, e in runs:
            s = hostapi.PCG(p, **kw)
            same_as_golden(collect(s, s.solve(itermax, float.fromhex(e["eps"]))), e, (kind, when))
            s.free()

    check("before")
    alive = hostapi.PCG(p, precond="mgpoly", levels=3, galerkin="device")
    alive.solve(20, 0.0)
    check("beside")
    alive.free()
    check("after")
    p.free()


CHILD = r"""
import sys
sys.path.insert(0, %r)
what = sys.argv[1]
from sparsebench_amd import capi, hostapi
import numpy as np
L = capi.init(0)
vp = hostapi.vp
ptr, col, val = hostapi.mg_trilinear(8, 8, 8)
nc = 64
if what == "sp":
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=1, precision="single")
elif what == "not_square":
    import ctypes
    rp, ci, v = np.array([0, 1, 2], np.uint32), np.array([0, 2], np.uint32), np.ones(2)
    m = L.sb_crs_upload(2, 3, rp.ctypes.data_as(vp), ci.ctypes.data_as(vp), v.ctypes.data_as(vp))
    ptr, col, val, nc = np.array([0, 1, 2], np.uint64), np.array([0, 0], np.uint32), np.ones(2), 1
    L.sb_matrix_galerkin(m, nc, ptr.ctypes.data_as(vp), col.ctypes.data_as(vp), val.ctypes.data_as(vp))
else:
    p = hostapi.Problem("generate", 8, 8, 8, fmt="scs", Cc=64, sigma=256)
if what == "column":
    col[100] = 64
if what == "pointer":
    ptr[201] = ptr[200] - 1
if what == "weight_nan":
    val[33] = np.nan
L.sb_matrix_galerkin(p.matrix, nc, ptr.ctypes.data_as(vp), col.ctypes.data_as(vp), val.ctypes.data_as(vp))
print("NOT REFUSED")
"""

REFUSALS = [("sp", "sb_matrix_galerkin: double precision only (the matrix was uploaded in single precision)"),
            ("not_square", "sb_matrix_galerkin: the matrix is not square (2 rows, 3 columns"),
            ("column", "sb_matrix_galerkin: level 0: the prolongation's row"),
            ("column", "has column 64 outside the 64 rows of level 1"),
            ("pointer", "sb_matrix_galerkin: level 0: the prolongation's row pointer falls from"),
            ("weight_nan", "has a weight that is not finite")]


@pytest.mark.parametrize("what,msg", REFUSALS)
def test_refusals_end_the_process_with_their_message(gpu, what, msg):
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT, what], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    err = out.stderr.decode()
    assert out.returncode == 1, (out.returncode, err[-1000:])
    assert msg in err and "sbhip:" in err and "NOT REFUSED" not in out.stdout.decode(), err[-1000:]
    assert "illegal memory access" not in err and "HIP error" not in err
