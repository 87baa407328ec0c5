"""solveCG on the GPU against the oracle and against histories captured from the
reference.

Parity chain (DESIGN.md "Parity"):
  1. GPU history == oracle history with the SAME fixed dot order: bit for bit.
  2. oracle with the reference's sequential dot == reference strict-IEEE build:
     bit for bit (tests/test_oracle_pinning.py, CPU).
  3. link 1 vs link 2 differ only by the summation order inside ddot; the
     deviation is bounded by the sequential sum's own rounding error and is
     checked here against the tolerance north_star names (1e-12 relative) on every
     case where that bound allows it.
"""
import os

import numpy as np
import pytest

from conftest import REFDATA, fused_levels, modes_scs
from oracle import pyoracle as po
from sparsebench_amd import hostapi

pytestmark = pytest.mark.gpu


def f(a):
    return np.array([float(v) for v in a])


def run_gpu(filename, n, fmt, Cc, sigma, itermax, eps=0.0, fused=True, pack_mode=None, pack_try=None, fuse_p=-1, fuse_alpha=-1, fuse_beta=-1):
    nx, ny, nz = n if isinstance(n, tuple) else (n, n, n)
    p = hostapi.Problem(filename, nx, ny, nz, fmt=fmt, Cc=Cc, sigma=sigma)
    if pack_mode is not None:
        assert p.use_packed(pack_mode) == pack_mode
    if pack_try is not None:
        p.use_packed(pack_try)  # clamped to what the matrix has (CRS: its pattern mirror, if any)
    cg = hostapi.CG(p, fused=fused, fuse_p=fuse_p, fuse_alpha=fuse_alpha, fuse_beta=fuse_beta)
    k = cg.solve(itermax, eps)
    rr, pap = cg.history()
    out = dict(k=k, rr=rr, pAp=pap, x=cg.solution(), err=cg.check_residual(), fuse_p=cg.fuse_p(), launches=cg.launches_per_body())
    cg.free(), p.free()
    return out


CONFIGS = [("crs", 64, 1), ("scs", 64, 1), ("scs", 64, 256), ("scs", 4, 1), ("scs", 128, 512)]


@pytest.mark.parametrize("fmt,Cc,sigma", CONFIGS)
@pytest.mark.parametrize("n", [8, (16, 12, 10), 32])
def test_history_bit_identical_to_oracle_same_dot_order(gpu, fmt, Cc, sigma, n):
    dims = n if isinstance(n, tuple) else (n, n, n)
    g = po.GMatrix.generate(*dims)
    o = po.cg(g, itermax=60, fmt=fmt, Cc=Cc, sigma=sigma, dot="tree", want_x=True)
    # default kernel choice and the other one (5: masked row programs, 0: reference layout); fused 1: five launches per
    # body, 0: reference op list
    combos = ((1, None), (0, None), (1, 0), (0, 5))
    for fused, pack_try in combos:
        r = run_gpu("generate", n, fmt, Cc, sigma, 60, fused=fused, pack_try=pack_try)
        assert r["k"] == o["k"]
        assert np.array_equal(r["rr"], o["rr"]), (fused, pack_try, "rr")
        assert np.array_equal(r["pAp"], o["pAp"]), (fused, pack_try, "pAp")
        assert np.array_equal(r["x"], o["x"][0]), (fused, pack_try, "x")
        assert r["err"] == o["max_err"]


@pytest.mark.parametrize("dims,fmt,sigma", [((16, 16, 16), "scs", 1), ((128, 128, 2), "scs", 256), ((128, 128, 2), "scs", 1), ((32, 32, 32), "scs", 256),
                                            ((128, 128, 2), "crs", 1), ((70, 3, 5), "scs", 1), ((20, 5, 33), "scs", 64), ((24, 20, 16), "scs", 4096)])
def test_p_update_inside_the_spmv_same_bits(gpu, dims, fmt, sigma):
    """round 3: where every chunk is a masked row program the default loop takes p = r + beta p (and the owed x update)
    INSIDE the SpMV launch (spmv_prog_fusep: 4 launches per body; mapped windows for sigma > 1, simple ones otherwise; the
    SKIPPAD instantiation behind the CRS mirror).  Same bits as the separate p update (sb_cg_set_fuse_p(s, 0)) and as the
    oracle -- history, iteration count, x, residual check -- also in pieces, with an early exit through eps, and for
    itermax 0..3 (no body / first body only: p = r + 0.0 * r)."""
    g = po.GMatrix.generate(*dims)
    o = po.cg(g, itermax=50, fmt=fmt, Cc=64, sigma=sigma, dot="tree", want_x=True)
    on = run_gpu("generate", dims, fmt, 64, sigma, 50, fuse_p=1)
    off = run_gpu("generate", dims, fmt, 64, sigma, 50, fuse_p=0, fuse_alpha=0, fuse_beta=0)
    assert off["fuse_p"] == 0 and off["launches"] == 5
    for r in (on, off):
        assert r["k"] == o["k"] and np.array_equal(r["rr"], o["rr"]) and np.array_equal(r["pAp"], o["pAp"])
        assert np.array_equal(r["x"], o["x"][0]) and r["err"] == o["max_err"]
    if dims[0] >= 128:
        assert on["fuse_p"] == 1 and on["launches"] == 3  # lines of >= 128 rows: every chunk a row program (+ the alpha step inside the r update)
    if not on["fuse_p"]:
        return
    p = hostapi.Problem("generate", *dims, fmt=fmt, Cc=64, sigma=sigma)
    cg = hostapi.CG(p, fuse_p=1)
    oe = po.cg(g, itermax=50, eps=1e-3, fmt=fmt, Cc=64, sigma=sigma, dot="tree", want_x=True)
    assert cg.solve(50, 1e-3) == oe["k"] < o["k"]
    rr, pap = cg.history()
    assert np.array_equal(rr, oe["rr"]) and np.array_equal(pap, oe["pAp"]) and np.array_equal(cg.solution(), oe["x"][0])
    cg.start(50, 0.0)  # in pieces: an odd and an even number of bodies behind the last piece (which p buffer is the newest)
    for piece in (1, 2, 4, 30, 12):
        cg.run_iters(piece)
    assert cg.finish() == o["k"]
    rr, pap = cg.history()
    assert np.array_equal(rr, o["rr"]) and np.array_equal(pap, o["pAp"]) and np.array_equal(cg.solution(), o["x"][0])
    for stop_after in (1, 2, 3, 8):  # finish() with bodies still outstanding: the owed x update uses the last p that was formed
        ok = po.cg(g, itermax=stop_after + 1, fmt=fmt, Cc=64, sigma=sigma, dot="tree", want_x=True)
        assert cg.solve(stop_after + 1, 0.0) == ok["k"]
        assert np.array_equal(cg.solution(), ok["x"][0]), stop_after
    for itermax in (0, 1, 2, 3):
        ok = po.cg(g, itermax=itermax, fmt=fmt, Cc=64, sigma=sigma, dot="tree", want_x=True)
        assert cg.solve(itermax, 0.0) == ok["k"] and np.array_equal(cg.history()[0], ok["rr"]) and np.array_equal(cg.solution(), ok["x"][0])
    cg.free(), p.free()


@pytest.mark.parametrize("dims,fmt,sigma,mode", [((8, 8, 8), "scs", 1, None), ((16, 12, 10), "crs", 1, None), ((33, 7, 5), "scs", 256, None),
                                                 ((32, 32, 32), "scs", 256, 0), ((128, 8, 4), "scs", 256, None), ((128, 8, 4), "scs", 1, 0),
                                                 ((48, 48, 48), "scs", 256, None)])
def test_scalar_steps_inside_their_consumers_same_bits(gpu, dims, fmt, sigma, mode):
    """round 3: on one rank the alpha step rides in the r update's launch and -- where the p update is a launch of its own -- the
    beta step / loop test at the head of the next body's p update (cg_update_r_k<1>, cg_update_p<1>: EVERY workgroup reduces the
    level-1 values itself, in the canonical order, workgroup 0 records the step): up to two launches fewer per loop body.  Same
    bits as the separate scalar launches (sb_cg_set_fuse_alpha / _beta(s, 0)) and as the oracle: history, k, x, residual check,
    an exit through eps, pieces (a step left owing at the end of a piece is taken by a launch of its own), itermax 0..3; with the
    reference-layout kernel (mode 0) and the row programs, n not a multiple of 256."""
    g = po.GMatrix.generate(*dims)
    o = po.cg(g, itermax=40, fmt=fmt, Cc=64, sigma=sigma, dot="tree", want_x=True)
    runs = {(a, b): run_gpu("generate", dims, fmt, 64, sigma, 40, pack_try=mode, fuse_alpha=a, fuse_beta=b) for a in (1, 0) for b in (1, 0)}
    for r in runs.values():
        assert r["k"] == o["k"] and np.array_equal(r["rr"], o["rr"]) and np.array_equal(r["pAp"], o["pAp"])
        assert np.array_equal(r["x"], o["x"][0]) and r["err"] == o["max_err"]
    base = runs[(0, 0)]["launches"]
    if not (fmt == "crs" and mode is None):  # (a CRS matrix without a mirror: level-0 partials from the dot pass, nothing folds)
        assert runs[(1, 0)]["launches"] == base - 1
        assert runs[(1, 1)]["launches"] == base - (1 if runs[(1, 1)]["fuse_p"] else 2)  # (p update inside the SpMV: the beta step stays)
    p = hostapi.Problem("generate", *dims, fmt=fmt, Cc=64, sigma=sigma)
    if mode is not None:
        p.use_packed(mode)
    cg = hostapi.CG(p, fuse_alpha=1, fuse_beta=1)
    oe = po.cg(g, itermax=40, eps=1e-2, fmt=fmt, Cc=64, sigma=sigma, dot="tree", want_x=True)
    assert cg.solve(40, 1e-2) == oe["k"]
    rr, pap = cg.history()
    assert np.array_equal(rr, oe["rr"]) and np.array_equal(pap, oe["pAp"]) and np.array_equal(cg.solution(), oe["x"][0])
    cg.start(40, 0.0)
    for piece in (1, 2, 4, 21, 12):
        cg.run_iters(piece)
    assert cg.finish() == o["k"]
    rr, pap = cg.history()
    assert np.array_equal(rr, o["rr"]) and np.array_equal(pap, o["pAp"]) and np.array_equal(cg.solution(), o["x"][0])
    for itermax in (0, 1, 2, 3):
        ok = po.cg(g, itermax=itermax, fmt=fmt, Cc=64, sigma=sigma, dot="tree", want_x=True)
        assert cg.solve(itermax, 0.0) == ok["k"] and np.array_equal(cg.history()[0], ok["rr"]) and np.array_equal(cg.history()[1], ok["pAp"])
        assert np.array_equal(cg.solution(), ok["x"][0])
    cg.free(), p.free()


def test_launches_per_body_variants(gpu):
    """fused = 1 (default): five launches per body; 0: the reference's op list; 2 and 3 (removed levels) behave as 1.
    Same bits in all of them, also when the loop is driven in pieces (every run_iters call flushes an owed beta step) and
    when it ends early (eps)."""
    g = po.GMatrix.generate(24, 20, 16)
    o = po.cg(g, itermax=70, fmt="scs", Cc=64, sigma=1, dot="tree", want_x=True)
    oe = po.cg(g, itermax=70, eps=1e-4, fmt="scs", Cc=64, sigma=1, dot="tree", want_x=True)
    assert oe["k"] < o["k"]
    for fused, want in ((1, 5), (0, 0), (3, 5), (2, 5)):
        p = hostapi.Problem("generate", 24, 20, 16, fmt="scs", Cc=64, sigma=1)
        cg = hostapi.CG(p, fused=fused, fuse_p=0, fuse_alpha=0, fuse_beta=0)  # (the p update inside the SpMV, the scalar steps inside their consumers: tests of their own)
        assert cg.launches_per_body() == want
        assert cg.solve(70, 0.0) == o["k"]
        rr, pap = cg.history()
        assert np.array_equal(rr, o["rr"]) and np.array_equal(pap, o["pAp"]) and np.array_equal(cg.solution(), o["x"][0])
        # in pieces: the loop state is complete after every piece
        cg.start(70, 0.0)
        done = 0
        for piece in (1, 1, 5, 30, 32):
            cg.run_iters(piece)
            done += piece
            c = cg.counters()
            assert c["n_pAp"] == done, (c, done, fused)
            if fused:  # (the reference's op list takes the loop test at the START of the next body)
                last = done == 69  # the 69th body's loop test fails (k = 70 = itermax): no further r.r, stop raised
                assert c["iters"] == (69 if last else done + 1) and c["n_rr"] == (69 if last else done + 1), (c, done, fused)
                assert c["stop"] == int(last), (c, done, fused)
        assert cg.finish() == o["k"]
        rr, pap = cg.history()
        assert np.array_equal(rr, o["rr"]) and np.array_equal(pap, o["pAp"]) and np.array_equal(cg.solution(), o["x"][0])
        # early exit through eps: the bodies enqueued behind the exit do nothing
        assert cg.solve(70, 1e-4) == oe["k"]
        rr, pap = cg.history()
        assert np.array_equal(rr, oe["rr"]) and np.array_equal(pap, oe["pAp"]) and np.array_equal(cg.solution(), oe["x"][0])
        cg.free(), p.free()


def test_band_klein_plumbing_case(gpu, golden_1rank):
    """configs[0]: exact solve after one step, r.r = [100, 0], NaN alpha, k = 3
     -- the reference's loop-exit semantics on the device"""
    gd = golden_1rank["band_klein"]
    path = os.path.join(REFDATA, "matrix_band_klein.mtx")
    for fmt, Cc, sg in CONFIGS:
        r = run_gpu(path, 1, fmt, Cc, sg, 150)
        assert r["k"] == gd["k"] == 3
        assert np.array_equal(r["rr"], f(gd["rr"])) and np.array_equal(r["pAp"], f(gd["pAp"]))
        assert np.all(np.isnan(r["x"]))  # alpha = 0/0 poisons x, as in the reference


def test_eps_stops_the_loop_like_the_reference(gpu):
    g = po.GMatrix.generate(12, 12, 12)
    for eps in (1e-3, 1e-9, 1e3, 1e9):
        o = po.cg(g, itermax=80, dot="tree", eps=eps)
        r = run_gpu("generate", 12, "scs", 64, 1, 80, eps=eps)
        assert r["k"] == o["k"], eps
        assert np.array_equal(r["rr"], o["rr"]) and np.array_equal(r["pAp"], o["pAp"]), eps
    for itermax in (0, 1, 2, 3):
        o = po.cg(g, itermax=itermax, dot="tree")
        r = run_gpu("generate", 12, "crs", 64, 1, itermax)
        assert r["k"] == o["k"] and np.array_equal(r["rr"], o["rr"]), itermax


def _rel(a, b):
    return np.abs(a - b) / np.abs(b)


@pytest.mark.parametrize("name,n,fmt,Cc,sigma", [
    ("hpcg8", 8, "crs", 64, 1), ("hpcg8", 8, "scs", 64, 1), ("hpcg16", 16, "scs", 64, 1),
    ("hpcg16", 16, "scs", 64, 256), ("hpcg32", 32, "scs", 64, 1), ("hpcg32", 32, "crs", 64, 1)])
def test_history_vs_reference_1e12(gpu, golden_1rank, name, n, fmt, Cc, sigma):
    """north_star: residual history within 1e-12 relative of the reference CPU CG.
    Holds on these sizes while the recurrence is above its own noise floor
    (r.r/r.r0 >= 1e-20, i.e. ten orders of residual reduction)."""
    gd = golden_1rank[name]
    ref_rr, ref_pap = f(gd["rr"]), f(gd["pAp"])
    r = run_gpu("generate", n, fmt, Cc, sigma, gd["itermax"])
    assert r["k"] == gd["k"] and len(r["rr"]) == len(ref_rr)
    live = ref_rr / ref_rr[0] >= 1e-20
    assert live.sum() >= 10
    TOL = 1e-12
    assert _rel(r["rr"], ref_rr)[live].max() <= TOL
    assert _rel(r["pAp"], ref_pap)[live[:len(ref_pap)]].max() <= TOL
    # and at every iteration the residual norm agrees to 1e-12 of the initial one
    assert (np.abs(np.sqrt(r["rr"]) - np.sqrt(ref_rr)) / np.sqrt(ref_rr[0])).max() <= TOL


def _exact(name):
    from conftest import load_json
    e = load_json("cg_hist_exact.json")[name]
    return f(e["rr"]), f(e["pAp"]), e


def _tree(key):
    """oracle history in the GPU's own dot order (tests/golden/cg_hist_tree.json, made by make_golden_tree.py): bit-for-bit target"""
    from conftest import load_json
    t = load_json("cg_hist_tree.json")[key]
    return f(t["rr"]), f(t["pAp"]), t


def _assert_bits(r, key):
    rr, pap, t = _tree(key)
    m, q = min(len(rr), len(r["rr"])), min(len(pap), len(r["pAp"]))
    assert m >= t["itermax"] - 2 or m == len(r["rr"])
    assert np.array_equal(r["rr"][:m], rr[:m]) and np.array_equal(r["pAp"][:q], pap[:q]), key


def test_history_64_against_exact_dots_and_reference(gpu, golden_1rank):
    """BASELINE configs[1] size.  tests/golden/cg_hist_exact.json = CG with every dot exactly rounded (Dot2,
    CPU, tests/golden/make_golden_exact.py).  The GPU stays within north_star's 1e-12 of it at every live
    iteration (observed 1e-14); the reference's own sequential sum does not (2.5e-11): at this size the
    reference is the outlier, and the GPU-vs-reference deviation is bounded at 2x what is observed."""
    gd = golden_1rank["hpcg64"]
    ref_rr = f(gd["rr"])
    ex_rr, ex_pap, ex = _exact("hpcg64")
    r = run_gpu("generate", 64, "scs", 64, 1, gd["itermax"])
    _assert_bits(r, "hpcg64_x1_scs_C64_sigma1")  # bit for bit against the oracle (tree order) at configs[1]'s size
    live = ex_rr / ex_rr[0] >= 1e-20
    d_gpu = _rel(r["rr"], ex_rr)[live].max()
    d_ref = _rel(ref_rr, ex_rr)[live].max()
    assert d_gpu <= 1e-12 and _rel(r["pAp"], ex_pap)[live[:len(ex_pap)]].max() <= 1e-12
    assert (np.abs(np.sqrt(r["rr"]) - np.sqrt(ex_rr)) / np.sqrt(ex_rr[0])).max() <= 1e-12
    assert d_ref > 100 * d_gpu and abs(d_ref - ex["reference_dev"]["rel"]) <= 1e-3 * d_ref
    # GPU vs the reference history itself: 2x the observed 2.5e-11 per iteration / 3.4e-12 normalised
    assert _rel(r["rr"], ref_rr)[live].max() <= 5e-11
    assert (np.abs(np.sqrt(r["rr"]) - np.sqrt(ref_rr)) / np.sqrt(ref_rr[0])).max() <= 7e-12


def test_full_size_properties_128(gpu, golden_1rank):
    """BASELINE configs[2] size (128^3, SCS C=64 sigma=256): size-independent checks.
    r.r0 closed form (exact in fp64), b = A*1 so CG converges to x = 1, SCS == CRS
    histories bit for bit under the same dot order, fused == unfused."""
    n = 128
    a = run_gpu("generate", n, "scs", 64, 1, 60)
    m = n - 2
    assert a["rr"][0] == m ** 3 + 600 * m ** 2 + 3072 * m + 3200
    _assert_bits(a, "hpcg128_x1_scs_C64_sigma1")  # bit for bit against the oracle (tree order) at the benchmark size
    c = run_gpu("generate", n, "crs", 64, 1, 60, pack_mode=0)  # native CRS kernel
    assert np.array_equal(a["rr"], c["rr"]) and np.array_equal(a["pAp"], c["pAp"])
    c3 = run_gpu("generate", n, "crs", 64, 1, 60, pack_mode=5)  # CRS through its pattern mirror's row programs (the default here)
    assert np.array_equal(c3["rr"], c["rr"]) and np.array_equal(c3["pAp"], c["pAp"]) and np.array_equal(c3["x"], c["x"])
    u = run_gpu("generate", n, "scs", 64, 1, 60, fused=False)
    assert np.array_equal(a["rr"], u["rr"]) and np.array_equal(a["x"], u["x"])
    s = run_gpu("generate", n, "scs", 64, 256, 60)
    _assert_bits(s, "hpcg128_x1_scs_C64_sigma256")  # ... configs[2] itself, default kernel
    _assert_bits(c, "hpcg128_x1_crs")
    # the benchmark configuration: every SpMV kernel the library has (reference layout and the default masked row programs)
    # gives the same bits
    for mode in [m for m in modes_scs() if m != 5]:
        q = run_gpu("generate", n, "scs", 64, 256, 25, pack_mode=mode)
        assert np.array_equal(q["rr"], s["rr"][:len(q["rr"])]) and np.array_equal(q["pAp"], s["pAp"][:len(q["pAp"])]), mode
    ref_rr = f(golden_1rank["hpcg128"]["rr"])
    ex_rr, ex_pap, ex = _exact("hpcg128")
    for r in (a, s):
        # against the exactly-rounded-dot history (cg_hist_exact.json): north_star's 1e-12 at every iteration
        assert _rel(r["rr"][:len(ex_rr)], ex_rr).max() <= 1e-12 and _rel(r["pAp"][:len(ex_pap)], ex_pap).max() <= 1e-12
        # the reference's sequential sum is the outlier (3.2e-10 from exact); GPU vs reference bounded at 2x observed
        assert _rel(ref_rr, ex_rr[:len(ref_rr)]).max() > 100 * _rel(r["rr"][:len(ex_rr)], ex_rr).max()
        assert _rel(r["rr"][:len(ref_rr)], ref_rr).max() <= 6.5e-10
        assert (np.abs(np.sqrt(r["rr"][:len(ref_rr)]) - np.sqrt(ref_rr)) / np.sqrt(ref_rr[0])).max() <= 8e-11
        assert np.all(np.diff(r["rr"][5:]) < 0)  # monotone once past the first steps
    long = run_gpu("generate", n, "scs", 64, 256, 150)
    assert long["err"] < 1e-6 and abs(long["x"] - 1.0).max() == long["err"]


def test_a_brick_eight_times_the_benchmark_size_256(gpu):
    """256^3 per GPU (16.8 M rows, 453 M stored elements: past the Infinity Cache, every chunk's columns span more than 16 bits,
    an x-line is exactly one 4-chunk tile): the library must still choose the masked row programs with the p update inside the
    SpMV (round 3: the LDS-window decision used to stop one step short at exactly this shape), and the loop on them must give the
    bits of the loop on the reference-layout kernel; closed-form r.r0 and p.Ap1 (exact integers at any size)."""
    from sparsebench_amd import knownanswers as ka
    n = 256
    p = hostapi.Problem("generate", n, n, n, fmt="scs", Cc=64, sigma=256)
    assert p.pack_info()["mode"] == 5
    cg = hostapi.CG(p)
    assert cg.fuse_p() == 1 and cg.launches_per_body() == 3
    cg.solve(12, 0.0)
    rr, pap = cg.history()
    assert rr[0] == ka.hpcg_rr0(n, n, n) and pap[0] == ka.hpcg_pAp1(n, n, n)
    cg.free()
    assert p.use_packed(0) == 0
    cg0 = hostapi.CG(p)
    cg0.solve(12, 0.0)
    rr0, pap0 = cg0.history()
    assert np.array_equal(rr, rr0) and np.array_equal(pap, pap0)
    cg0.free(), p.free()


def test_multi_rank_kernel_sequence_through_rccl_on_one_gpu(gpu, monkeypatch):
    """SB_FORCE_RCCL=1 attaches a 1-rank RCCL communicator: the CG then takes the
    multi-rank path (local reduce -> ncclAllReduce on the stream -> scalar update) and
    ddot / commReduction go through RCCL.  Same bits as the single-rank path."""
    import ctypes
    L = gpu
    base = run_gpu("generate", 16, "scs", 64, 256, 40)
    monkeypatch.setenv("SB_FORCE_RCCL", "1")
    raw = (ctypes.c_ubyte * 128)()
    L.sb_comm_unique_id(raw)
    L.sb_comm_init(0, 1, raw)
    try:
        assert L.sb_comm_size() == 1 and L.sb_comm_rank() == 0
        r = run_gpu("generate", 16, "scs", 64, 256, 40)
        u = run_gpu("generate", 16, "crs", 64, 1, 40, fused=False)
        from sparsebench_amd.capi import DeviceVector
        x = np.random.default_rng(0).standard_normal(5000)
        dx = DeviceVector.from_host(x)
        assert L.sb_ddot(len(x), dx.ptr, dx.ptr) == po.ddot_tree(x, x)
        one = DeviceVector.from_host(np.array([3.5]))
        L.sb_comm_reduction(one.ptr, 0)
        L.sb_comm_reduction(one.ptr, 1)
        assert one.get()[0] == 3.5
        L.sb_comm_barrier()
        dx.free(), one.free()
    finally:
        L.sb_comm_finalize()
    assert np.array_equal(r["rr"], base["rr"]) and np.array_equal(r["pAp"], base["pAp"])
    assert np.array_equal(r["x"], base["x"]) and r["k"] == base["k"]
    o = po.cg(po.GMatrix.generate(16, 16, 16), itermax=40, dot="tree")
    assert np.array_equal(u["rr"], o["rr"])


@pytest.mark.parametrize("first,second", [(0, 5), (5, 0)])
def test_a_kernel_mode_change_between_pieces_of_one_solve_cannot_mix_the_two_p_paths(gpu, first, second):
    """the p-update plan (inside the SpMV launch with p double-buffered, or in place) is latched by sb_cg_start.  If
    sb_matrix_use_packed / sb_cg_set_fuse_p is called between two sb_cg_run_iters pieces, the solve keeps the plan it started
    with -- 3 in-place bodies followed by a fused one used to read the zeroed second p buffer -- and the change applies from the
    next sb_cg_start.  History and x equal the undisturbed solve, bit for bit."""
    n, iters = 32, 14
    p = hostapi.Problem("generate", n, n, n, fmt="scs", Cc=64, sigma=256)
    if p.use_packed(5) != 5:
        p.free()
        pytest.skip("no row programs for this matrix")
    assert p.use_packed(first) == first
    ref = hostapi.CG(p)
    plan = ref.fuse_p()
    ref.solve(iters, 0.0)
    rr0, pap0 = ref.history()
    x0 = ref.solution()
    ref.free()
    cg = hostapi.CG(p)
    cg.start(iters, 0.0)
    cg.run_iters(3)
    assert p.use_packed(second) == second  # mid-solve: kernel mode of the matrix changes ...
    cg.L.sb_cg_set_fuse_p(cg.ptr, 1 if second else 0)  # ... and so does the wish
    assert cg.fuse_p() == plan             # ... the running solve keeps its plan
    cg.run_iters(4)
    assert p.use_packed(first) == first
    cg.run_iters(iters)
    cg.finish()
    rr, pap = cg.history()
    assert np.array_equal(rr, rr0) and np.array_equal(pap, pap0) and np.array_equal(cg.solution(), x0)
    cg.free(), p.free()
