"""Worker of tests/test_gpu_halo_fold.py: P processes share GPU 0 (gloo as the host-mediated transport, SB_P2P=1 for the
peer-mapped plane, as tests/gpu_multirank_worker.py) and solve every case twice -- sb_comm_halo_fold(0), then (1) -- on the
reference-layout Sell-64 kernel (mode 0).  Both solves must give k, the r.r and p.Ap histories, x and the residual check of
the P-rank restatement BIT FOR BIT (fp64: oracle/pyoracle.py with dot="tree", rank_sum="tree"; fp32: tests/sp_mpi_ref.py),
and report their launch counts: 7 / 5 per body where the fold engages, unchanged where it must not.

argv: PRECISION(double|single) VARIANT FMT C SIGMA NAME ITERMAX
  VARIANT  fold     the fold must engage with the switch on
           crs | mode5 | fused0 | seq | nohalo   it must NOT engage (nohalo: the test sets SB_P2P_HALO=0)
           split    start / run_iters(3) / flip the switch / run_iters / finish: the body a solve started with is kept
  NAME     hpcgN, irregularN (the irregular stand-in at N^3 nodes), band_klein"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import pyoracle as po  # noqa: E402
from sparsebench_amd import capi, gloo_transport, hostapi  # noqa: E402
from irregular_locs import irregular_locs  # noqa: E402
import sp_mpi_ref  # noqa: E402

BAND = os.path.join(ROOT, "tests", "golden", "ref", "matrix_band_klein.mtx")


def bits(a, single):
    """the values' bit patterns, every NaN as one pattern"""
    if single:
        a = np.asarray(a, np.float32)
        return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))
    a = np.asarray(a, np.float64)
    return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))


def main():
    dist.init_process_group("gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    precision, variant, fmt, Cc, sigma, name, itermax = (sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]),
                                                        sys.argv[6], int(sys.argv[7]))
    single = precision == "single"
    os.environ.setdefault("SB_SHARED_GPU", "1")  # every rank on the one GPU
    L = capi.init(0)
    H = hostapi.host(precision)
    keep = gloo_transport.attach(L, H, dist, rank, size)  # noqa: F841  (ctypes callbacks must stay alive)
    assert L.sb_comm_halo_fold_selected() == 0  # the default

    # the problem and its P-rank restatement
    if name == "band_klein":
        filename, n = BAND, 1
    elif name.startswith("irregular"):
        filename, n = "irregular", int(name[9:])
    else:
        filename, n = "generate", int(name[4:])
    prob = hostapi.Problem(filename, n, n, n, fmt=fmt, Cc=Cc, sigma=sigma, rank=rank, size=size, precision=precision)
    order = "seq" if variant == "seq" else "tree"
    fused = variant != "fused0"
    if single:
        locs, plans, keep2 = sp_mpi_ref.locals_and_plans(po, BAND if name == "band_klein" else name, size)
        orders = None
        if fmt == "scs" and sigma > 1:  # the tree dot runs over the device's row order
            allo = [None] * size
            dist.all_gather_object(allo, prob.array("newToOldPerm").astype(np.int64).tolist())
            orders = [np.array(o, np.int64) for o in allo]
        k0, rr0, pap0, x0 = sp_mpi_ref.cg(locs, plans, itermax, dot=order, orders=orders)
        err0 = None
    else:
        if name == "band_klein":
            locs = [po.GMatrix.from_mtx(BAND, r, size) for r in range(size)]
        elif name.startswith("irregular"):
            locs = irregular_locs(n, size)
        else:
            locs = [po.GMatrix.generate(n, n, n, r, size) for r in range(size)]
        plans = po.Plans(locs)
        o = po.cg(locs, plans, itermax=itermax, fmt=fmt, Cc=Cc, sigma=sigma, dot=order, rank_sum="tree", want_x=True)
        k0, rr0, pap0, x0, err0 = o["k"], o["rr"], o["pAp"], o["x"], o["max_err"]

    # the kernel: the reference layout (mode 0) -- except where the variant asks for the row programs
    if not single:
        got = prob.use_packed(5 if variant == "mode5" else 0)
        if variant == "mode5":
            assert got == 5, "rank %d: the matrix has no row programs: the mode-5 case would be vacuous" % rank
    halo_p2p = L.sb_halo_p2p_enabled(prob.halo)
    engage = variant in ("fold", "split") and bool(halo_p2p)

    def check(cg, k, what):
        rr, pap = cg.history()
        x = cg.solution()
        err = cg.check_residual()
        assert k == k0, (what, rank, k, k0)
        assert np.array_equal(bits(rr, single), bits(rr0, single)), ("rr",) + what
        assert np.array_equal(bits(pap, single), bits(pap0, single)), ("pAp",) + what
        if name != "band_klein" or single:  # (fp64 band_klein: alpha = 0/0 poisons x with NaN; compared between the two solves)
            assert np.array_equal(bits(x, single), bits(x0[rank], single)), ("x",) + what
        if err0 is not None and name != "band_klein":
            assert err == err0, ("check_residual",) + what
        return bits(rr, single), bits(pap, single), bits(x, single), bits([err], single)

    if variant == "split":
        for first in (1, 0):  # the switch at the start; flipped after three bodies
            L.sb_comm_halo_fold(first)
            cg = hostapi.CG(prob, fused=True, dot_order="tree")
            cg.start(itermax, 0.0)
            want = 1 if (first and engage) else 0
            assert cg.halo_fold() == want, (first, cg.halo_fold())
            cg.run_iters(3)
            L.sb_comm_halo_fold(1 - first)
            assert cg.halo_fold() == want, (first, cg.halo_fold())  # the running solve keeps its body
            if halo_p2p:
                assert cg.launches_per_body() == (5 if want else 7), (first, cg.launches_per_body())
            cg.run_iters(itermax - 1 - 3)
            k = cg.finish()
            check(cg, k, ("split", first, rank))
            if halo_p2p:  # the next solve follows the switch as it stands now
                assert cg.halo_fold() == (1 - first), (first, cg.halo_fold())
            cg.free()
            print("FOLD_SPLIT rank %d started_with %d kept %d" % (rank, first, want), flush=True)
        L.sb_comm_halo_fold(0)
    else:
        seen = {}
        for fold in (0, 1):
            L.sb_comm_halo_fold(fold)
            assert L.sb_comm_halo_fold_selected() == fold
            cg = hostapi.CG(prob, fused=fused, dot_order=order)
            hf, lpb, cpb = cg.halo_fold(), cg.launches_per_body(), cg.collectives_per_body()
            k = cg.solve(itermax, 0.0)
            seen[fold] = (hf, lpb, cpb) + check(cg, k, (variant, "fold=%d" % fold, rank))
            cg.free()
            print("FOLD_COUNTS rank %d fold %d halo_fold %d launches %d collectives %d" % (rank, fold, hf, lpb, cpb), flush=True)
        L.sb_comm_halo_fold(0)
        for i in range(3, 7):  # on == off, NaNs and the residual included
            assert np.array_equal(seen[0][i], seen[1][i]), ("on vs off", i, rank)
        if engage:
            assert seen[0][:3] == (0, 7, 0), seen[0][:3]
            assert seen[1][:3] == (1, 5, 0), seen[1][:3]
        elif variant != "fold":  # must not engage: nothing changes
            assert seen[0][0] == 0 and seen[1][0] == 0, (seen[0][:3], seen[1][:3])
            assert seen[0][1:3] == seen[1][1:3], (seen[0][:3], seen[1][:3])

    dist.barrier()
    p2p = L.sb_comm_p2p_enabled()
    flags = torch.tensor([p2p, halo_p2p], dtype=torch.int32)
    lo, hi = flags.clone(), flags.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    assert torch.equal(lo, hi), "ranks disagree on the data plane: %r vs %r" % (lo.tolist(), hi.tolist())
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
        print("HALO_FOLD_OK", " ".join(sys.argv[1:]), size, flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
