"""The reference's dot order on several ranks (tests/gpu_dot_order_worker.py): P processes share GPU 0 through
torch.distributed / gloo, on both data planes -- the in-kernel all-reduce over peer-mapped memory (SB_P2P=1) and the
communicator's (SB_P2P=0) -- and reproduce the MPI reference's histories (tests/golden/cg_hist_mpi.json) bit for bit."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("p2p", ["1", "0"])
@pytest.mark.parametrize("key,size", [("hpcg16_x2", 2), ("hpcg16_x4", 4), ("hpcg8_x8", 8), ("band_klein_x2", 2)])
def test_seq_order_reproduces_the_mpi_reference(gpu, key, size, p2p):
    env = dict(os.environ, OMP_NUM_THREADS="1", SB_P2P=p2p)
    env.pop("SB_DOT_ORDER", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(size),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "gpu_dot_order_worker.py"), key]
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-4000:]
    assert "GPU_DOT_ORDER_OK %s %d" % (key, size) in text, text[-3000:]
    for fmt in ("crs", "scs"):
        assert "DOT_ORDER_CASE_OK %s %s" % (key, fmt) in text
    if p2p == "0":
        assert "p2p 0" in text  # the communicator's all-reduce really ran
