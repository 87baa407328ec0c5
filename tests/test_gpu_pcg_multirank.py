"""Preconditioned CG on several ranks on one GPU: P processes (one rank each) share GPU 0 and talk through the
host-mediated gloo transport, launched exactly as tests/test_gpu_multirank.py launches its worker (tests/gpu_pcg_multirank_worker.py
is this file's).  Every solve -- Jacobi, a caller's diagonal, the Chebyshev polynomial -- equals the P-rank restatement
(tests/pcg_mpi_ref.py) bit for bit on both data planes; with dinv = 1 it equals hostapi.CG of the same processes.  Plus the
new local-reduce kernel in one process, and the refusals."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "gpu_pcg_multirank_worker.py")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch(size, args, **env):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(size),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), WORKER] + [str(a) for a in args]
    out = subprocess.run(cmd, env=dict(os.environ, OMP_NUM_THREADS="1", SB_P2P_REPORT="1", **env), stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=900)
    return out.returncode, out.stdout.decode()


def plane_used(text, p2p):
    """the plane the ranks REALLY ran on, as tests/test_gpu_multirank.py judges it: a peer-mapped case that fell back on this box
    is skipped with the reason, not passed"""
    why = [ln for ln in text.splitlines() if ln.startswith(("P2P_REASON", "HALO_P2P_REASON"))]
    if p2p == "0":
        assert "P2P_ENABLED 0" in text and "HALO_P2P_ENABLED 0" in text
        assert any("SB_P2P=0" in ln for ln in why), why
    else:
        if "P2P_ENABLED 1" not in text or "HALO_P2P_ENABLED 1" not in text:
            pytest.skip("peer-mapped path fell back on this box: %s" % why)
        assert any(ln.startswith("P2P_REASON on:") for ln in why) and any(ln.startswith("HALO_P2P_REASON on:") for ln in why), why


# fmt, C, sigma, n per rank, P, itermax, workload: the smallest shapes at which each thing can still go wrong
CASES = [
    ("scs", 64, 256, 16, 2, 100, "generate"),   # permuted rows, halo pack through the permutation
    ("scs", 64, 1, 16, 4, 100, "generate"),     # interior ranks with two neighbours, full pairwise tree
    ("crs", 64, 1, 16, 2, 100, "generate"),     # native CRS, the separate dot pass
    ("scs", 4, 8, 8, 3, 100, "generate"),       # generic C, odd P, and the tree's odd tail
    ("crs", 64, 1, 12, 3, 100, "irregular"),    # every rank a neighbour of every other; rows scaled differently: Jacobi matters
    ("scs", 64, 256, 12, 3, 100, "irregular"),
]


@pytest.mark.parametrize("p2p", ["1", "0"])
@pytest.mark.parametrize("fmt,Cc,sigma,n,size,itermax,workload", CASES)
def test_pcg_on_several_ranks_is_the_restatement_bit_for_bit(gpu, fmt, Cc, sigma, n, size, itermax, workload, p2p):
    """p2p=1: pcg_scalar_p2p_k (one value in the alpha step, two back to back in the prologue's and the beta step) and the push and
    pull launches; p2p=0: local reduce | one transport all-reduce per value | step, and pack | send / recv.  Same bits."""
    rc, text = launch(size, [fmt, Cc, sigma, n, itermax, workload, "solves"], SB_P2P=p2p)
    assert rc == 0, text[-4000:]
    assert "GPU_PCG_MULTIRANK_OK solves %s %d %d %d %d" % (fmt, Cc, sigma, n, size) in text, text[-3000:]
    if workload == "irregular":
        assert "INDEGREE 2" in text
    plane_used(text, p2p)


def test_p2p_setup_failure_on_one_rank_runs_pcg_on_the_communicators_plane(gpu):
    """the existing host-side set-up failure (SB_P2P_FAIL_RANK): every rank ends on the communicator's plane and still equals the
    restatement"""
    rc, text = launch(3, ["scs", 64, 1, 16, 60, "generate", "solves"], SB_P2P="1", SB_P2P_FAIL_RANK="1")
    assert rc == 0, text[-4000:]
    assert "GPU_PCG_MULTIRANK_OK solves scs 64 1 16 3" in text and "P2P_ENABLED 0" in text, text[-3000:]
    assert text.count("in-kernel all-reduce over peer-mapped memory: off") == 3


def test_cg_and_pcg_alternate_on_the_shared_sequence_counter(gpu):
    """a hostapi.CG solve and a hostapi.PCG solve on the same handles, twice: CG advances the exchange counter by one per dot, PCG
    by one or two per scalar step, and every solve still equals its reference"""
    rc, text = launch(2, ["scs", 64, 256, 16, 40, "generate", "alternate"], SB_P2P="1")
    assert rc == 0, text[-4000:]
    assert "GPU_PCG_MULTIRANK_OK alternate scs 64 256 16 2" in text, text[-3000:]
    plane_used(text, "1")


@pytest.mark.parametrize("scenario,msg", [
    ("refuse_sgs", "sb_pcg_create_sgs: PCG runs on one rank (this process is rank"),
    ("refuse_plan", "sb_pcg_create: the halo plan receives"),
])
def test_refusals_on_two_ranks_end_the_processes_with_their_message(gpu, scenario, msg):
    """in child processes, as tests/test_gpu_pcg.py checks its refusals: fatal with file:line, no GPU fault"""
    rc, text = launch(2, ["crs", 64, 1, 8, 10, "generate", scenario], SB_P2P="0")
    assert rc != 0, text[-2000:]
    assert msg in text and "sbhip:" in text and "NOT REFUSED" not in text, text[-3000:]
    assert "illegal memory access" not in text and "HIP error" not in text


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70000])
def test_local_reduce_kernel_is_levels_1_and_2(gpu, n):
    """pcg_local_reduce_k through its native entry against numpy's restatement of levels 1-2 (level 0 by the oracle's
    ddot_partials, as tests/pcg_ref.update_r takes it): both sums, the one-sum form, and a stopped loop, which leaves the block
    alone"""
    from oracle import pyoracle as po
    from sparsebench_amd.capi import DeviceVector
    L = gpu
    rng = np.random.RandomState(n)
    a, b = rng.standard_normal(n), rng.standard_normal(n) * 2.0 ** rng.randint(-20, 20, n)

    def levels_1_2(q):
        """thread t adds level-1 values t, t + 1024, ... in order; each wave's 64 by the xor butterfly; the 16 wave sums in order"""
        s = np.zeros(1024)
        for i, v in enumerate(q):
            s[i % 1024] = s[i % 1024] + v
        w = s.reshape(16, 64)
        for off in (1, 2, 4, 8, 16, 32):
            w = w + w[:, np.arange(64) ^ off]
        total = w[0, 0]
        for k in range(1, 16):
            total = total + w[k, 0]
        return total

    want = levels_1_2(po.ddot_partials(a, b)), levels_1_2(po.ddot_partials(a, a))
    assert want == (po.reduce_final(po.ddot_partials(a, b)), po.reduce_final(po.ddot_partials(a, a)))  # the oracle's own levels 1-2
    da, db = DeviceVector.from_host(a), DeviceVector.from_host(b)
    out = (C.c_double * 2)()
    L.sb_pcg_local_reduce_native(n, 1, 0, da.ptr, db.ptr, out)
    assert (out[0], out[1]) == want
    L.sb_pcg_local_reduce_native(n, 0, 0, da.ptr, db.ptr, out)
    assert (out[0], out[1]) == (want[0], -2.0)
    L.sb_pcg_local_reduce_native(n, 1, 1, da.ptr, db.ptr, out)
    assert (out[0], out[1]) == (-1.0, -2.0)
