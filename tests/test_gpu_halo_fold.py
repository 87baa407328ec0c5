"""The halo exchange folded into the streaming CG loop's own kernels (sb_comm_halo_fold / SB_HALO_FOLD): P processes share
GPU 0 over the gloo transport with the peer-mapped plane on (tests/gpu_halo_fold_worker.py).  Every case is solved with the
switch off and on; both solves must equal the P-rank restatement bit for bit -- k, r.r and p.Ap histories, x, residual
check -- and where the fold engages the body is 5 launches (cg_update_p_push | spmv_scs64_halo | alpha | r update | beta)
instead of 7, with no communicator call.  Where it must not engage nothing changes.  No tolerance anywhere."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "gpu_halo_fold_worker.py")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run(size, args, extra_env=None, timeout=900):
    env = dict(os.environ, OMP_NUM_THREADS="1", SB_P2P="1", SB_P2P_REPORT="1", SB_SHARED_GPU="1")
    for k in ("SB_HALO_FOLD", "SB_HALO_PUSH_INSIDE", "SB_P2P_HALO", "SB_DOT_ORDER"):
        env.pop(k, None)
    env.update(extra_env or {})
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(size), "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), WORKER] + [str(a) for a in args]
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout + 30)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-4000:]
    assert "HALO_FOLD_OK " + " ".join(str(a) for a in args) + " %d" % size in text, text[-3000:]
    return text


def _need_peer_mapped_plane(text):
    """a silent fall-back of the peer-mapped set-up must not pass as a folded run"""
    why = [ln for ln in text.splitlines() if ln.startswith(("P2P_REASON", "HALO_P2P_REASON"))]
    if "P2P_ENABLED 1" not in text or "HALO_P2P_ENABLED 1" not in text:
        pytest.skip("peer-mapped path fell back on this box: %s" % why)


def _counts(text, size, fold, halo_fold, launches):
    for r in range(size):
        assert "FOLD_COUNTS rank %d fold %d halo_fold %d launches %d collectives 0" % (r, fold, halo_fold, launches) in text, text[-3000:]


# (fmt, C, sigma, problem, ranks, itermax): the sizes and iteration counts of tests/test_gpu_multirank.py
FP64 = [
    ("scs", 64, 256, "hpcg16", 2, 100),      # permuted rows: the send list through the device order
    ("scs", 64, 1, "hpcg16", 4, 100),        # interior ranks with two neighbours
    ("scs", 64, 1, "hpcg48", 3, 150),        # several chunks per plane, many exchanges: both parities of the staging area
    ("scs", 64, 256, "hpcg128", 2, 20),      # the benchmark's brick; sigma > 1 with a device permutation
    ("scs", 64, 256, "irregular12", 3, 40),  # every rank a neighbour of every other, many halo blocks
    ("scs", 64, 1, "band_klein", 2, 150),    # the NaN exit at k = 3 with a push just sent
]
FP32 = [
    ("scs", 64, 256, "hpcg16", 2, 100),
    ("scs", 64, 1, "hpcg16", 4, 100),
    ("scs", 64, 1, "hpcg48", 3, 150),
    ("scs", 64, 1, "band_klein", 2, 150),
]


@pytest.mark.parametrize("fmt,Cc,sigma,name,size,itermax", FP64)
def test_fold_fp64(gpu, fmt, Cc, sigma, name, size, itermax):
    text = _run(size, ["double", "fold", fmt, Cc, sigma, name, itermax])
    _need_peer_mapped_plane(text)
    _counts(text, size, 0, 0, 7)
    _counts(text, size, 1, 1, 5)
    if name.startswith("irregular"):
        assert "INDEGREE 2" in text, text[-3000:]


@pytest.mark.parametrize("fmt,Cc,sigma,name,size,itermax", FP32)
def test_fold_fp32(gpu, fmt, Cc, sigma, name, size, itermax):
    text = _run(size, ["single", "fold", fmt, Cc, sigma, name, itermax])
    _need_peer_mapped_plane(text)
    _counts(text, size, 0, 0, 7)
    _counts(text, size, 1, 1, 5)


# where the fold must not engage: halo_fold() == 0 with the switch on, the launch counts and the bits of the switch off
@pytest.mark.parametrize("variant,fmt,env", [
    ("crs", "crs", None),
    ("mode5", "scs", None),
    ("fused0", "scs", None),
    ("seq", "scs", None),
    ("nohalo", "scs", {"SB_P2P_HALO": "0"}),
])
def test_fold_does_not_engage(gpu, variant, fmt, env):
    text = _run(2, ["double", variant, fmt, 64, 1, "hpcg16", 100], env)
    if variant != "nohalo":
        _need_peer_mapped_plane(text)
    else:
        assert "HALO_P2P_ENABLED 0" in text, text[-3000:]
    for r in range(2):
        for fold in (0, 1):
            assert "FOLD_COUNTS rank %d fold %d halo_fold 0 " % (r, fold) in text, text[-3000:]


@pytest.mark.parametrize("precision", ["double", "single"])
def test_a_running_solve_keeps_its_body(gpu, precision):
    """start / run_iters(3) / flip the switch / run_iters / finish: the plan is latched per solve"""
    text = _run(2, [precision, "split", "scs", 64, 1, "hpcg16", 60])
    _need_peer_mapped_plane(text)
    for r in range(2):
        assert "FOLD_SPLIT rank %d started_with 1 kept 1" % r in text and "FOLD_SPLIT rank %d started_with 0 kept 0" % r in text, text[-3000:]

