"""The single-precision mirror on several ranks on one MI355X: the existing worker of tests/test_gpu_sp_multirank.py
(tests/gpu_sp_multirank_worker.py, unchanged) with SB_SP_MIRROR=1, so that every rank's upload builds the float mirror and
every SpMV of its solves is spmv_prog_f32 behind the float halo exchange.  The worker's own assertions -- the numpy P-rank
restatement in the tree order fused and unfused and in seq, the launch counts of DESIGN 6's SP row -- pass unchanged on both
data planes, and SB_SP_MIRROR_REPORT proves inside the worker processes that the mirror was built."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "gpu_sp_multirank_worker.py")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run(size, args, p2p, timeout):
    env = dict(os.environ, OMP_NUM_THREADS="1", SB_P2P=p2p, SB_P2P_REPORT="1", SB_SHARED_GPU="1", SB_SP_MIRROR="1",
               SB_SP_MIRROR_REPORT="1")
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(size), "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), WORKER] + args
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout + 30)
    return out.returncode, out.stdout.decode()


@pytest.mark.parametrize("p2p", ["1", "0"])
def test_sp_cg_on_two_ranks_through_the_mirror(gpu, p2p):
    """hpcg128 on 2 ranks, Sell-64-256 (for fp64 every rank's chunks are all row programs at this size:
    tests/test_gpu_multirank.py): a built=0 fails, it does not skip.  12 iterations in two dot orders: the worker's numpy
    restatement costs seconds per rank and SpMV at this size"""
    size, itermax = 2, 12
    rc, text = _run(size, ["cg", "scs", "64", "256", "hpcg128", str(itermax)], p2p, 900)
    assert rc == 0, text[-4000:]
    assert "SP_MULTIRANK_OK cg scs 64 256 hpcg128 %d %d" % (itermax, size) in text, text[-3000:]
    report = [ln for ln in text.splitlines() if "SP_MIRROR built=" in ln]
    assert len(report) == size, report
    assert all("SP_MIRROR built=1 fmt=scs" in ln for ln in report), report
    if p2p == "0":
        assert "P2P_ENABLED 0" in text and "HALO_P2P_ENABLED 0" in text


def test_a_small_problem_with_the_switch_on_passes_as_before(gpu):
    """the control: hpcg16 on 2 ranks with the switch on, whatever it reports"""
    rc, text = _run(2, ["cg", "scs", "64", "256", "hpcg16", "100"], "1", 300)
    assert rc == 0, text[-4000:]
    assert "SP_MULTIRANK_OK cg scs 64 256 hpcg16 100 2" in text and "GOLDEN_SEQ_OK hpcg16_x2" in text, text[-3000:]
    assert len([ln for ln in text.splitlines() if "SP_MIRROR built=" in ln]) == 2
