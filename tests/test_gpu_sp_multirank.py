"""Single-precision CG on several ranks on one MI355X: P processes share GPU 0 (tests/gpu_sp_multirank_worker.py) with the gloo
transport and SB_SHARED_GPU=1.  Every case runs on both data planes -- the peer-mapped one (float halo push / pull, the in-kernel
float all-reduce inside the scalar step) and the communicator's (halo pack widened for the host transport, local reduce |
all-reduce | apply) -- and must give the same bits: the numpy P-rank restatement in the tree order, fused and unfused, and the
reference's own SP MPI histories in the seq order (tests/golden/cg_hist_sp_mpi.json)."""
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


def _run(size, args, env, timeout):
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(size), "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), WORKER] + args
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout + 30)
    return out.returncode, out.stdout.decode()


# (fmt, C, sigma, problem, ranks, itermax, seconds)
CASES = [
    ("scs", 64, 256, "hpcg16", 2, 100, 300),     # permuted rows: the tree over the device order, the push through packIdx
    ("scs", 64, 1, "hpcg16", 4, 100, 300),       # interior ranks with two neighbours
    ("crs", 64, 1, "hpcg16", 2, 100, 300),       # the level-1 dot pass behind the SpMV
    ("scs", 4, 8, "hpcg8", 3, 40, 300),          # generic C, an odd rank count: (v0 + v1) + v2
    ("scs", 64, 1, "hpcg48", 3, 150, 600),       # many exchanges: staging-area parity and flags
    ("scs", 64, 1, "band_klein", 2, 150, 300),
    ("crs", 64, 1, "hpcg8", 8, 60, 600),         # the reference's 8-rank history
    ("scs", 64, 1, "hpcg7x7x9", 3, 40, 300),     # a 7 x 7 x 9 brick per rank, 441 rows (n % 4 = 1): float halo push / pull and p update over a partial float4
]
GOLDEN = {("hpcg16", 2): "hpcg16_x2", ("hpcg16", 4): "hpcg16_x4", ("hpcg8", 8): "hpcg8_x8", ("band_klein", 2): "band_klein_x2"}


def _check_plane(p2p, text):
    why = [ln for ln in text.splitlines() if ln.startswith(("P2P_REASON", "HALO_P2P_REASON"))]
    if p2p == "0":
        assert "P2P_ENABLED 0" in text and "HALO_P2P_ENABLED 0" in text
        assert any("SB_P2P=0" in ln for ln in why), why
    elif "P2P_ENABLED 1" not in text or "HALO_P2P_ENABLED 1" not in text:
        # the peer-mapped kernels must really have run -- a silent fall-back would make the parametrisation vacuous
        pytest.skip("peer-mapped path fell back on this box: %s" % why)


@pytest.mark.parametrize("p2p", ["1", "0"])
@pytest.mark.parametrize("fmt,Cc,sigma,name,size,itermax,seconds", CASES)
def test_sp_cg_on_several_ranks(gpu, fmt, Cc, sigma, name, size, itermax, seconds, p2p):
    env = dict(os.environ, OMP_NUM_THREADS="1", SB_P2P=p2p, SB_P2P_REPORT="1", SB_SHARED_GPU="1")
    rc, text = _run(size, ["cg", fmt, str(Cc), str(sigma), name, str(itermax)], env, seconds)
    assert rc == 0, text[-4000:]
    assert "SP_MULTIRANK_OK cg %s %d %d %s %d %d" % (fmt, Cc, sigma, name, itermax, size) in text, text[-3000:]
    if (name, size) in GOLDEN:
        assert "GOLDEN_SEQ_OK " + GOLDEN[(name, size)] in text, text[-3000:]
    _check_plane(p2p, text)


@pytest.mark.parametrize("fmt,Cc,sigma,name,size", [("scs", 64, 256, "hpcg16", 2), ("scs", 64, 1, "hpcg16", 4), ("crs", 64, 1, "hpcg8", 3)])
def test_sp_reference_shaped_ops(gpu, fmt, Cc, sigma, name, size):
    env = dict(os.environ, OMP_NUM_THREADS="1", SB_P2P_REPORT="1", SB_SHARED_GPU="1")
    rc, text = _run(size, ["ops", fmt, str(Cc), str(sigma), name, "1"], env, 300)
    assert rc == 0, text[-4000:]
    assert "SP_MULTIRANK_OK ops" in text, text[-3000:]


def test_sp_transport_without_allgather_is_refused_at_setup(gpu):
    """the float all-reduce needs the transport's allgather_bytes: without it the SP upload ends every rank with the message
    (before any kernel of the run; no rank waits for another)"""
    env = dict(os.environ, OMP_NUM_THREADS="1", SB_SHARED_GPU="1")
    rc, text = _run(2, ["noallgather"], env, 300)
    assert rc != 0 and rc not in (124, 137), text[-3000:]
    assert "needs its allgather_bytes callback" in text and "sb_scs_upload_f32" in text, text[-3000:]
    assert "NOALLGATHER_UNEXPECTED" not in text
