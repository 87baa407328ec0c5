"""Worker of tests/test_gpu_pcg_multirank.py: P processes share GPU 0 and run preconditioned CG on several ranks
through the product's own path -- partition, upload, halo plan, sb_pcg_create / sb_pcg_create_poly with the plan, the loop with
the halo exchange ahead of every SpMV and the paired all-reduce --, with torch.distributed / gloo as the host transport
(sparsebench_amd/gloo_transport.py), launched as tests/gpu_multirank_worker.py is.  Every solve must equal the P-rank
restatement (tests/pcg_mpi_ref.py) bit for bit in k, r.r, r.z, p.Ap and this rank's x.

argv: fmt C sigma n itermax workload scenario
  scenario "solves": Jacobi, a caller's diagonal, the polynomial at 1 and 3 steps and at 3 steps with a caller's lmax, with
      eps = 0; Jacobi and the 3-step polynomial again to eps = 1e-10 ||b||; dinv = 1 against hostapi.CG; the launch and
      collective counts; in every kernel mode the matrix has
  scenario "alternate": a hostapi.CG solve and a hostapi.PCG solve on the same handles, twice (the shared sequence counter)
  scenario "refuse_sgs" / "refuse_plan": the refusals, which end every rank's process
"""
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyoracle as po  # noqa: E402
from sparsebench_amd import capi, gloo_transport, hostapi  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pcg_mpi_ref as ref  # noqa: E402
from pcg_ref import same_bits  # noqa: E402

vp = C.c_void_p


def agree(values, what):
    """every rank holds the same doubles / ints"""
    t = torch.tensor([float(v) for v in values], dtype=torch.float64)
    lo, hi = t.clone(), t.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    assert torch.equal(lo, hi), "ranks disagree on %s: %r vs %r" % (what, lo.tolist(), hi.tolist())


def check(tag, s, k, want, rank):
    rr, rz, pap = s.history()
    x = s.solution()
    assert k == want["k"], (tag, "k", k, want["k"])
    assert same_bits(rr, want["rr"]), (tag, "rr", rank)
    assert same_bits(rz, want["rz"]), (tag, "rz", rank)
    assert same_bits(pap, want["pAp"]), (tag, "pAp", rank)
    assert same_bits(x, want["x"][rank]), (tag, "x", rank)


def expected_counts(L, prob, fused_dot, steps):
    """(launches, collectives) per body as include/sbhip.h documents them: steps = 0 the diagonal, else the polynomial's"""
    p2p, halo_p2p = L.sb_comm_p2p_enabled(), L.sb_halo_p2p_enabled(prob.halo)
    base = (5 if fused_dot else 6) + (2 * (steps - 1) if steps else 0)
    exchanges = steps if steps else 1
    per = (int(prob.totalSendCount > 0) + int(prob.indegree > 0)) if halo_p2p else int(prob.totalSendCount > 0)
    return base + exchanges * per + (0 if p2p else 2), (0 if p2p else 3) + (0 if halo_p2p else exchanges)


def main():
    dist.init_process_group("gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    fmt, Cc, sigma, n, itermax = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    workload, scenario = sys.argv[6], sys.argv[7]
    os.environ.setdefault("SB_SHARED_GPU", "1")  # every rank on the one GPU: no placement search
    L = capi.init(0)
    H = hostapi.host()
    keep = gloo_transport.attach(L, H, dist, rank, size)  # noqa: F841  (ctypes callbacks must stay alive)
    prob = hostapi.Problem(workload, n, n, n, fmt=fmt, Cc=Cc, sigma=sigma, rank=rank, size=size)
    b, xe = prob.rhs()

    if scenario == "refuse_sgs":  # past hostapi.PCG's own ValueError: the library's refusal
        L.sb_pcg_create_sgs(prob.matrix, prob.halo, b.ctypes.data_as(vp), None)
        print("NOT REFUSED", flush=True)
        return
    if scenario == "refuse_plan":  # a matrix of the plan's nr rows with one halo column more than the plan receives
        nr = prob.nr
        rowPtr, col, val = np.arange(nr + 1, dtype=np.uint32), np.arange(nr, dtype=np.uint32), np.full(nr, 4.0)
        m = L.sb_crs_upload(nr, prob.nc + 1, rowPtr.ctypes.data_as(vp), col.ctypes.data_as(vp), val.ctypes.data_as(vp))
        L.sb_pcg_create(m, prob.halo, b.ctypes.data_as(vp), None, None)
        print("NOT REFUSED", flush=True)
        return

    try:  # hostapi's own refusal, on a real two-rank Problem, before the library
        hostapi.PCG(prob, precond="sgs")
        raise AssertionError("hostapi.PCG(precond='sgs') was not refused on %d ranks" % size)
    except ValueError as e:
        assert "runs on one rank (the problem is rank %d of %d)" % (rank, size) in str(e), e
    R = (ref.Ranks.irregular if workload == "irregular" else ref.Ranks.generate)(n, size, fmt, Cc, sigma)
    jac, caller, ones = R.jacobi(), ref.caller_dinv(R), [np.ones(g.nr) for g in R.locs]
    eps = 1e-10 * R.norm_b()

    if scenario == "alternate":
        want_cg = po.cg(R.locs, R.plans, itermax=itermax, fmt=fmt, Cc=Cc, sigma=sigma, dot="tree", rank_sum="tree", want_x=True)
        want_pcg = ref.solve(R, jac, itermax, 0.0)
        cg, pcg = hostapi.CG(prob, fused=1), hostapi.PCG(prob)
        for turn in range(2):
            k = cg.solve(itermax, 0.0)
            rr, pap = cg.history()
            assert k == want_cg["k"] and same_bits(rr, want_cg["rr"]) and same_bits(pap, want_cg["pAp"]), ("cg", turn, rank)
            assert same_bits(cg.solution(), want_cg["x"][rank]), ("cg x", turn, rank)
            check("pcg turn %d" % turn, pcg, pcg.solve(itermax, 0.0), want_pcg, rank)
        cg.free(), pcg.free()
    else:
        # the reference once: it does not depend on the kernel mode
        lmax_own = float(R.lmax(R.to_dev(jac))) * 1.25  # a caller's lmax: the same double on every rank
        runs = [("jacobi", dict(dinv=jac[rank]), jac, None, 0.0), ("caller", dict(dinv=caller[rank]), caller, None, 0.0),
                ("poly1", dict(precond="poly", steps=1), jac, dict(steps=1), 0.0),
                ("poly3", dict(precond="poly", steps=3), jac, dict(steps=3), 0.0),
                ("poly3_lmax", dict(precond="poly", steps=3, lmax=lmax_own), jac, dict(steps=3, lmax=lmax_own), 0.0),
                ("jacobi_eps", dict(), jac, None, eps), ("poly3_eps", dict(precond="poly", steps=3), jac, dict(steps=3), eps)]
        wants = {tag: ref.solve(R, dinv, itermax, e, poly=poly) for tag, _, dinv, poly, e in runs}
        want_one = ref.solve(R, ones, itermax, 0.0)
        exits = [tag for tag, _, _, _, e in runs if e > 0.0 and 1 < wants[tag]["k"] < itermax]
        assert exits, "no run leaves the loop at eps before itermax = %d: %r" % (itermax, {t: wants[t]["k"] for t in wants})
        for mode in ((5, 0) if (fmt == "scs" and Cc == 64) or fmt == "crs" else (0,)):
            got_mode = prob.use_packed(mode)  # clamped to what the matrix has
            fused_dot = (fmt == "scs" and Cc == 64) or got_mode >= 1
            for tag, kw, _, poly, e in runs:
                s = hostapi.PCG(prob, **kw)
                check("%s mode %d" % (tag, mode), s, s.solve(itermax, e), wants[tag], rank)
                if xe is not None and np.all(xe == 1.0):  # max|x - xexact| over EVERY rank's rows
                    assert s.check_residual() == max(float(np.max(np.abs(xq - 1.0))) for xq in wants[tag]["x"]), (tag, "max_err")
                else:
                    assert xe is None and s.check_residual() == 0.0
                want_counts = expected_counts(L, prob, fused_dot, poly["steps"] if poly else 0)
                assert (s.launches_per_body(), s.collectives_per_body()) == want_counts, (tag, mode, s.launches_per_body(),
                                                                                          s.collectives_per_body(), want_counts)
                if poly:
                    iv = s.interval()
                    assert iv == wants[tag]["interval"], (tag, iv, wants[tag]["interval"])
                    agree(iv, "sb_pcg_poly_interval")
                    assert same_bits(s.coeffs(), wants[tag]["coeffs"])
                s.free()
            # dinv = 1: sb_cg in the tree order of the same processes, GPU against GPU (and the restatement)
            s, cg = hostapi.PCG(prob, dinv=ones[rank]), hostapi.CG(prob, fused=1)
            k, kc = s.solve(itermax, 0.0), cg.solve(itermax, 0.0)
            rr, rz, pap = s.history()
            crr, cpap = cg.history()
            assert k == kc and same_bits(rr, crr) and same_bits(rz, rr) and same_bits(pap, cpap), ("identity", mode, rank)
            assert same_bits(s.solution(), cg.solution()), ("identity x", mode, rank)
            check("identity mode %d" % mode, s, k, want_one, rank)
            s.free(), cg.free()

    dist.barrier()
    p2p, halo_p2p = L.sb_comm_p2p_enabled(), L.sb_halo_p2p_enabled(prob.halo)
    agree([p2p, halo_p2p], "the data plane")
    why, why_halo = L.sb_comm_p2p_reason().decode(), L.sb_halo_p2p_reason(prob.halo).decode()
    indegree = prob.indegree
    prob.free()
    L.sb_comm_finalize()
    if rank == 0:
        print("P2P_ENABLED", p2p, flush=True)
        print("HALO_P2P_ENABLED", halo_p2p, flush=True)
        print("P2P_REASON", why, flush=True)
        print("HALO_P2P_REASON", why_halo, flush=True)
        print("INDEGREE", indegree, flush=True)
        print("GPU_PCG_MULTIRANK_OK", scenario, fmt, Cc, sigma, n, size, flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
