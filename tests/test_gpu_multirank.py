"""The N-rank DEVICE path on one GPU: several processes (one rank each) share GPU 0 and
talk through a host-mediated gloo transport instead of RCCL (see
tests/gpu_multirank_worker.py).  Covers what the 1-GPU box cannot reach with RCCL: halo
pack indices through the SCS permutation, halo columns in the compressed stream / LDS
windows, received entries landing in the tail of p, the split local-reduce / all-reduce /
scalar-step sequence, and the device-side loop exit on every rank."""
import os
import re
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


CASES = [
    ("scs", 64, 256, 16, 2, 100),   # permuted rows, compressed stream + LDS windows with halo segments
    ("scs", 64, 1, 16, 4, 100),     # interior ranks with two neighbours
    ("crs", 64, 1, 16, 2, 100),
    ("scs", 4, 8, 8, 3, 40),        # generic-C kernel, odd rank count
    ("scs", 64, 1, 48, 3, 150),     # several tiles per rank, many exchanges: staging-area parity, flags, row patterns
    ("scs", 64, 256, 128, 2, 20),   # BASELINE configs[3]'s brick (128^3 per rank, Sell-64-256), two ranks on the one GPU
]
# every case on both data planes; the push-inside variant of the peer-mapped halo on the Sell-64 cases with 16^3 and 48^3 per rank
PARAMS = [c + (p,) for p in ("1", "0") for c in CASES] + [c + ("push-inside",) for c in CASES if c[0] == "scs" and c[1] == 64 and c[3] in (16, 48)]


@pytest.mark.parametrize("fmt,Cc,sigma,n,size,itermax,p2p", PARAMS)
def test_device_multirank_path(gpu, fmt, Cc, sigma, n, size, itermax, p2p):
    """p2p=1: the dot all-reduces happen inside the scalar step over peer-mapped (IPC) memory when the
    ranks' kernels really run concurrently on the one GPU (otherwise the self-test falls back, which the
    worker reports); p2p=0: local reduce | transport all-reduce | scalar step.  Same bits either way."""
    # p2p=1 (the default set-up): push kernel + SpMV whose halo-touching tiles wait for the flags themselves;
    # p2p=0: transport send-recv
    # "push-inside": p2p = 1 with the halo push carried by the first workgroups of the SpMV launch (SB_HALO_PUSH_INSIDE=1)
    inside = p2p == "push-inside"
    if inside:
        p2p = "1"
    env = dict(os.environ, OMP_NUM_THREADS="1", SB_P2P=p2p, SB_P2P_REPORT="1", SB_HALO_PUSH_INSIDE="1" if inside else "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(size),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "gpu_multirank_worker.py"), fmt, str(Cc), str(sigma), str(n), str(itermax)]
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-4000:]
    assert "GPU_MULTIRANK_OK %s %d %d %d %d" % (fmt, Cc, sigma, n, size) in text, text[-3000:]
    if (fmt, Cc, n) == ("scs", 64, 128):
        # BASELINE configs[3]'s brick: EVERY rank's matrix -- also the one whose halo plane lies below its first rows --
        # gets the default pattern kernel (level 6) for all of its chunks (halo columns in ascending global order inside
        # the private windows: sb_set_external_ids from commPartition)
        progs = re.findall(r"ROW_PROGRAMS rank (\d+) (\d+) of (\d+)", text)
        assert len(progs) == size and all(int(a) == int(b) > 0 for _, a, b in progs), progs
    why = [ln for ln in text.splitlines() if ln.startswith(("P2P_REASON", "HALO_P2P_REASON"))]
    if p2p == "0":
        assert "P2P_ENABLED 0" in text and "HALO_P2P_ENABLED 0" in text
        assert any("SB_P2P=0" in ln for ln in why), why
    else:
        # the peer-mapped kernels (cg_scalar_p2p_k, halo_push_k, the HALO instantiation of the pattern SpMV) must
        # really have run on every rank -- a silent fall-back would make this parametrisation vacuous
        if "P2P_ENABLED 1" not in text or "HALO_P2P_ENABLED 1" not in text:
            pytest.skip("peer-mapped path fell back on this box: %s" % why)
        assert any(ln.startswith("P2P_REASON on:") for ln in why) and any(ln.startswith("HALO_P2P_REASON on:") for ln in why), why


@pytest.mark.parametrize("fmt,sigma", [("crs", 1), ("scs", 256)])
def test_irregular_stand_in_on_three_ranks(gpu, fmt, sigma):
    """configs[4]'s stand-in split over 3 ranks on the one GPU: its far couplings make every rank a neighbour of every
    other (indegree 2), no pattern levels apply (native CRS / reference-layout Sell-64-sigma kernels inside the multi-rank
    loop, the CRS one with the separate dot pass), halo push / pull and in-kernel all-reduce over peer-mapped memory.
    History, x and residual bit-identical to the oracle's 3-rank run."""
    env = dict(os.environ, OMP_NUM_THREADS="1", SB_P2P="1", SB_P2P_REPORT="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "gpu_multirank_worker.py"), fmt, "64", str(sigma), "12", "40", "irregular"]
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-4000:]
    assert "GPU_MULTIRANK_OK %s 64 %d 12 3" % (fmt, sigma) in text and "INDEGREE 2" in text, text[-3000:]


def test_p2p_setup_failure_on_one_rank_falls_back_everywhere(gpu):
    """the in-kernel all-reduce is enabled collectively: if ONE rank cannot export / map its buffer, every
    rank must end up on the transport's all-reduce (no rank may wait in a kernel for a peer that never
    writes), and the run is still bit-exact"""
    env = dict(os.environ, OMP_NUM_THREADS="1", SB_P2P="1", SB_P2P_FAIL_RANK="1", SB_P2P_REPORT="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "gpu_multirank_worker.py"), "scs", "64", "1", "16", "60"]
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-4000:]
    assert "GPU_MULTIRANK_OK scs 64 1 16 3" in text and "P2P_ENABLED 0" in text, text[-3000:]
    assert text.count("in-kernel all-reduce over peer-mapped memory: off") == 3
    assert "P2P_REASON off:" in text and ("rank 1" in text.split("P2P_REASON off:")[1].splitlines()[0]
                                           or "another rank" in text.split("P2P_REASON off:")[1].splitlines()[0])
