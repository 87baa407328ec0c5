"""Worker of tests/test_gpu_sp_multirank.py: P processes share GPU 0 and run single-precision CG on P ranks through the product
(SP host library: partition -> _f32 upload -> halo plan -> sb_cg_create_f32), with torch.distributed/gloo as the host-mediated
transport (sparsebench_amd/gloo_transport.py) and, where its set-up succeeds, the peer-mapped plane (SB_P2P).

  cg CASE...   tree order fused and unfused: k, history and x bit-equal to the numpy P-rank restatement (tests/sp_mpi_ref.py);
               seq order: bit-equal to the restatement and, where the case is one of tests/golden/cg_hist_sp_mpi.json, to the
               reference's own SP MPI history; the launch count of the fused body on the plane in use
  ops CASE...  sb_halo_exchange_f32 puts the exact float of the owning rank's row in every tail slot (device row order, sigma > 1
               included); sb_comm_reduction_f32 SUM / MAX equal the pairwise float tree
  noallgather  a transport without allgather_bytes: the SP upload must end the process with its message
CASE = fmt C sigma name itermax (name: hpcgN, hpcgXxYxZ or band_klein)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import pyoracle as po  # noqa: E402
from sparsebench_amd import capi, gloo_transport, hostapi  # noqa: E402
import sp_mpi_ref  # noqa: E402

vp = C.c_void_p
F = np.float32
BAND = os.path.join(ROOT, "tests", "golden", "ref", "matrix_band_klein.mtx")


def bits(a):
    a = np.asarray(a, F)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def problem(fmt, Cc, sigma, name, rank, size):
    if name == "band_klein":
        return hostapi.Problem(BAND, 1, 1, 1, fmt=fmt, Cc=Cc, sigma=sigma, rank=rank, size=size, precision="single")
    nx, ny, nz = sp_mpi_ref.hpcg_dims(name)
    return hostapi.Problem("generate", nx, ny, nz, fmt=fmt, Cc=Cc, sigma=sigma, rank=rank, size=size, precision="single")


def run_cg(L, prob, fmt, Cc, sigma, name, itermax, rank, size):
    locs, plans, keep = sp_mpi_ref.locals_and_plans(po, BAND if name == "band_klein" else name, size)
    orders = None
    if fmt == "scs" and sigma > 1:  # the tree dot runs over the device's row order
        allo = [None] * size
        dist.all_gather_object(allo, prob.array("newToOldPerm").astype(np.int64).tolist())
        orders = [np.array(o, np.int64) for o in allo]
    for order in ("tree", "seq"):
        k0, rr0, pap0, x0 = sp_mpi_ref.cg(locs, plans, itermax, dot=order, orders=orders)
        for fused in ((True, False) if order == "tree" else (True,)):
            cg = hostapi.CG(prob, fused=fused, dot_order=order)
            k = cg.solve(itermax, 0.0)
            rr, pap = cg.history()
            x = cg.solution()
            lpb = cg.launches_per_body()
            cg.check_residual()  # (commReduction MAX in float: one more all-reduce, the same on every rank)
            cg.free()
            what = (order, fused, rank)
            assert k == k0, (what, k, k0)
            assert np.array_equal(bits(rr), bits(rr0)), ("rr",) + what
            assert np.array_equal(bits(pap), bits(pap0)), ("pAp",) + what
            assert np.array_equal(bits(x), bits(x0[rank])), ("x",) + what
            if order == "tree" and fused:
                p2p, hp2p = L.sb_comm_p2p_enabled(), L.sb_halo_p2p_enabled(prob.halo)
                want = 5 if (fmt == "scs" and Cc == 64) else 6  # p update | SpMV | (dot pass) | alpha | r update | beta
                if hp2p:
                    want += (prob.totalSendCount > 0) + (prob.indegree > 0)  # push, pull
                else:
                    want += (prob.totalSendCount > 0) + (prob.externalCount > 0)  # pack, the host transport's unpack
                want += 0 if p2p else 2  # local reduce | all-reduce | apply
                assert lpb == want, (lpb, want, p2p, hp2p)
            if order == "seq":
                assert lpb == 0
                key = "%s_x%d" % (name, size)
                golden = json.load(open(os.path.join(ROOT, "tests", "golden", "cg_hist_sp_mpi.json")))
                if key in golden and golden[key]["itermax"] == itermax:
                    g = golden[key]
                    assert k == g["k"]
                    assert np.array_equal(bits(rr), bits([float(v) for v in g["rr"]])), ("golden rr", rank)
                    assert np.array_equal(bits(pap), bits([float(v) for v in g["pAp"]])), ("golden pAp", rank)
                    if rank == 0:
                        print("GOLDEN_SEQ_OK", key, flush=True)
    for loc in locs:
        loc.free()


def run_ops(L, prob, fmt, sigma, name, rank, size):
    locs, plans, keep = sp_mpi_ref.locals_and_plans(po, BAND if name == "band_klein" else name, size)
    first = int(locs[rank].startRow)
    nr, nc = prob.nr, prob.nr + prob.externalCount
    val = lambda gid: (np.asarray(gid, np.float64) * 0.5 + 0.25).astype(F)  # exact floats, one per global row
    orig = val(first + np.arange(nr))
    dev = orig[prob.array("newToOldPerm").astype(np.int64)] if fmt == "scs" and sigma > 1 else orig  # the vector's device order
    host = np.concatenate([dev, np.full(nc - nr, F(-7.0))]).astype(F)
    d = L.sb_malloc(nc * 4 + 4)
    L.sb_h2d(d, host.ctypes.data_as(vp), nc * 4)
    L.sb_halo_exchange_f32(prob.halo, d)
    L.sb_sync()
    out = np.empty(nc, F)
    L.sb_d2h(out.ctypes.data_as(vp), d, nc * 4)
    L.sb_free(d)
    assert np.array_equal(bits(out[:nr]), bits(dev)), rank
    assert np.array_equal(bits(out[nr:]), bits(val(prob.array("externalGlobal")))), rank
    # the float all-reduce: the same value sets on every rank, rank r contributes element r
    rng = np.random.default_rng(size)
    tiny = F(1.4e-45)
    sets = [rng.standard_normal(size).astype(F), (rng.integers(1, 1000, size) * tiny).astype(F),
            np.array([(1e8 if i % 2 == 0 else -1e8) + i for i in range(size)], F), np.array([1.0] + [2.0 ** -24] * (size - 1), F)]
    s = L.sb_malloc(8)
    for v in sets:
        for op, ref in ((1, sp_mpi_ref.rank_sum), (0, sp_mpi_ref.rank_max)):
            mine = np.array([v[rank]], F)
            L.sb_h2d(s, mine.ctypes.data_as(vp), 4)
            L.sb_comm_reduction_f32(s, op)
            L.sb_sync()
            L.sb_d2h(mine.ctypes.data_as(vp), s, 4)
            assert bits(mine)[0] == bits(ref(list(v))), (op, v, mine, rank)
    L.sb_free(s)
    for loc in locs:
        loc.free()


def main():
    dist.init_process_group("gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    what = sys.argv[1]
    os.environ.setdefault("SB_SHARED_GPU", "1")  # every rank on the one GPU
    L = capi.init(0)
    H = hostapi.host("single")  # commPartition of the SP host library runs over this exchange
    keep = gloo_transport.attach(L, H, dist, rank, size, allgather_bytes=what != "noallgather")  # noqa: F841
    if what == "noallgather":
        problem("scs", 64, 1, "hpcg8", rank, size)  # must not return
        print("NOALLGATHER_UNEXPECTED rank %d" % rank, flush=True)
        return
    fmt, Cc, sigma, name, itermax = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], int(sys.argv[6])
    prob = problem(fmt, Cc, sigma, name, rank, size)
    if what == "cg":
        run_cg(L, prob, fmt, Cc, sigma, name, itermax, rank, size)
    else:
        run_ops(L, prob, fmt, sigma, name, rank, size)
    dist.barrier()
    p2p, halo_p2p = L.sb_comm_p2p_enabled(), L.sb_halo_p2p_enabled(prob.halo)
    why, why_halo = L.sb_comm_p2p_reason().decode(), L.sb_halo_p2p_reason(prob.halo).decode()
    prob.free()
    L.sb_comm_finalize()
    if rank == 0:
        print("P2P_ENABLED", p2p, flush=True)
        print("HALO_P2P_ENABLED", halo_p2p, flush=True)
        print("P2P_REASON", why, flush=True)
        print("HALO_P2P_REASON", why_halo, flush=True)
        print("SP_MULTIRANK_OK", what, " ".join(sys.argv[2:]), size, flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
