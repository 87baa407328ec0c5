"""Worker of tests/test_gpu_dot_order_multirank.py: P processes share GPU 0 (gloo as a host-mediated transport, as in
tests/gpu_multirank_worker.py) and solve in the reference's dot order (CG(dot_order="seq")): each rank's sequential sum
over its own rows, the ranks' sums combined by the library's all-reduce.  History must equal the reference under
mpiexec -n P (tests/golden/cg_hist_mpi.json) bit for bit, and the oracle's P-rank run with dot="seq", rank_sum="tree"."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyoracle as po  # noqa: E402
from sparsebench_amd import capi, gloo_transport, hostapi  # noqa: E402


def main():
    dist.init_process_group("gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    key = sys.argv[1]  # a case of cg_hist_mpi.json: hpcg<n>_x<P> or band_klein_x2
    os.environ.setdefault("SB_SHARED_GPU", "1")
    L = capi.init(0)
    H = hostapi.host()
    keep = gloo_transport.attach(L, H, dist, rank, size)  # noqa: F841  (ctypes callbacks must stay alive)
    import json
    gd = json.load(open(os.path.join(ROOT, "tests", "golden", "cg_hist_mpi.json")))[key]
    assert gd["ranks"] == size
    itermax = gd["itermax"]
    if key.startswith("band_klein"):
        path = os.path.join(ROOT, "tests", "golden", "ref", "matrix_band_klein.mtx")
        filename, n = path, 1
        locs = [po.GMatrix.from_mtx(path, r, size) for r in range(size)]
    else:
        n = int(key[4:].split("_")[0])
        filename = "generate"
        locs = [po.GMatrix.generate(n, n, n, r, size) for r in range(size)]
    plans = po.Plans(locs)
    ref_rr, ref_pap = np.array([float(v) for v in gd["rr"]]), np.array([float(v) for v in gd["pAp"]])
    for fmt, sigma in (("crs", 1), ("scs", 1)):
        o = po.cg(locs, plans, itermax=itermax, fmt=fmt, Cc=64, sigma=sigma, dot="seq", rank_sum="tree", want_x=True)
        assert np.array_equal(o["rr"], ref_rr) and np.array_equal(o["pAp"], ref_pap), ("oracle", fmt)
        prob = hostapi.Problem(filename, n, n, n, fmt=fmt, Cc=64, sigma=sigma, rank=rank, size=size)
        cg = hostapi.CG(prob, dot_order="seq")
        assert cg.dot_order() == "seq" and cg.launches_per_body() == 0 and cg.collectives_per_body() == 0
        k = cg.solve(itermax, 0.0)
        rr, pap = cg.history()
        x = cg.solution()
        cg.free()
        assert k == o["k"], (k, o["k"])
        assert np.array_equal(rr, ref_rr), ("rr vs the MPI reference", fmt, rank)
        assert np.array_equal(pap, ref_pap), ("pAp vs the MPI reference", fmt, rank)
        if not key.startswith("band_klein"):  # (band_klein: alpha = 0/0 poisons x with NaN)
            assert np.array_equal(x, o["x"][rank]), ("x", fmt, rank)
        plane = (L.sb_comm_p2p_enabled(), L.sb_halo_p2p_enabled(prob.halo))
        prob.free()
        if rank == 0:
            print("DOT_ORDER_CASE_OK %s %s p2p %d halo_p2p %d" % (key, fmt, plane[0], plane[1]), flush=True)
    dist.barrier()
    L.sb_comm_finalize()
    if rank == 0:
        print("GPU_DOT_ORDER_OK", key, size, flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
