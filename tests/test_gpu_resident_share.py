"""The resident share of the Sell-64 stream (sb_matrix_resident_share): k sixteenths of the 4-chunk blocks are read
with plain loads and stay in the Infinity Cache, the rest non-temporally.  Which loads a block uses must never change a bit:
SpMV, fused dot and CG histories at every share equal share 0 and the oracle.  The rule that picks the share is host
arithmetic and is tested without a device.  No tolerance anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_json
from oracle import pyoracle as po
from sparsebench_amd import capi, hostapi

import gpu_resident_share_worker as spmv_worker
from test_gpu_halo_fold import _counts, _free_port, _need_peer_mapped_plane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
PRODUCTS = 4 * 2 * 2 * len(spmv_worker.SHARES)  # matrices x sigmas x (ordinary, non-finite x[0]) x shares


@pytest.mark.gpu
def test_spmv_bits_at_every_share_xcd_mapping_on(gpu):
    if os.environ.get("SB_SCS_XCD") not in (None, "1"):
        pytest.fail("SB_SCS_XCD is set: this test is the XCD-mapped half")
    assert spmv_worker.check_spmv(gpu) == PRODUCTS


@pytest.mark.gpu
def test_spmv_bits_at_every_share_xcd_mapping_off(gpu):
    env = dict(os.environ, SB_SCS_XCD="0")
    out = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(HERE, "gpu_resident_share_worker.py")], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=150)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-4000:]
    assert "RESIDENT_SHARE_SPMV_OK xcd=0 products=%d" % PRODUCTS in text, text[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("sigma", [1, 256])
def test_cg_bits_at_every_share(gpu, sigma):
    """16^3, 20 iterations: x and both histories at shares 5 and 16 equal share 0, the oracle in the same dot order, and the
    committed tree-order history where there is one for the case"""
    prob = hostapi.Problem("generate", 16, 16, 16, fmt="scs", Cc=64, sigma=sigma)
    assert prob.use_packed(0) == 0
    o = po.cg(po.GMatrix.generate(16, 16, 16), itermax=20, fmt="scs", Cc=64, sigma=sigma, dot="tree", want_x=True)
    golden = load_json("cg_hist_tree.json").get("hpcg16_x1_scs_C64_sigma%d" % sigma)
    first = None
    for k in (0, 5, 16):
        assert prob.resident_share(k) == k
        cg = hostapi.CG(prob)
        its = cg.solve(20, 0.0)
        rr, pap = cg.history()
        x = cg.solution()
        cg.free()
        assert its == o["k"], (k, its, o["k"])
        assert np.array_equal(rr, o["rr"]) and np.array_equal(pap, o["pAp"]), ("histories vs the oracle", k)
        assert np.array_equal(x.view(np.uint64), o["x"][0].view(np.uint64)), ("x vs the oracle", k)
        if golden is not None:
            assert [float(v) for v in golden["rr"]][:len(rr)] == list(rr), ("committed history", k)
        if first is None:
            first = (rr, pap, x)
        assert np.array_equal(rr, first[0]) and np.array_equal(pap, first[1]) and np.array_equal(x.view(np.uint64), first[2].view(np.uint64)), ("vs share 0", k)
    prob.free()


@pytest.mark.gpu
def test_the_rule_is_the_default_and_comes_back(gpu):
    L = gpu
    prob = hostapi.Problem("generate", 16, 16, 16, fmt="scs", Cc=64, sigma=1)
    rule = L.sb_resident_share_rule(12.0 * prob.nElems, prob.nc, 1 if os.environ.get("SB_SHARED_GPU", "0") not in ("", "0") else 0)
    assert prob.resident_share(-1) == rule  # what the upload set
    assert prob.resident_share(5) == 5
    assert prob.resident_share(-1) == rule
    assert prob.resident_share(16) == 16 and prob.resident_share(0) == 0 and prob.resident_share(-1) == rule
    prob.free()
    crs = hostapi.Problem("generate", 8, 8, 8, fmt="crs")
    assert crs.resident_share(5) == 0  # not a matrix spmv_scs64 serves
    crs.free()


def test_the_rule():
    """host arithmetic only: share bytes = fill x (256 MiB - 4 vectors of nc doubles), rounded down to sixteenths of the stream"""
    L = capi.load()
    nr = 128 ** 3
    # HPCG 27-point at 128^3: sigma 1 pads every chunk to 27 entries per row; a sorted matrix (sigma 256) stores a little less
    for elems in (27 * nr, int(26.2 * nr)):
        k = L.sb_resident_share_rule(12.0 * elems, nr, 0)
        assert 0 < k < 16, (elems, k)
        assert k / 16.0 * 12.0 * elems + 4 * 8 * nr < 256 * 2 ** 20, "share and vectors must fit the cache together"
        assert L.sb_resident_share_rule(12.0 * elems, nr, 1) == 0  # ranks share the device
    nr = 256 ** 3
    assert L.sb_resident_share_rule(12.0 * 27 * nr, nr, 0) == 0  # the vectors alone exceed the cache
    assert L.sb_resident_share_rule(12.0 * 27 * 64 ** 3, 64 ** 3, 1) == 0
    assert L.sb_resident_share_rule(0.0, 0, 0) == 0
    # monotone in the room the vectors leave, never more than the stream
    ks = [L.sb_resident_share_rule(12.0 * 27 * 128 ** 3, nc, 0) for nc in (1 << 20, 1 << 21, 1 << 22, 1 << 23)]
    assert ks == sorted(ks, reverse=True) and ks[-1] == 0, ks
    assert L.sb_resident_share_rule(1e6, 1000, 0) == 16


@pytest.mark.gpu
def test_halo_twin_at_share_5(gpu):
    """spmv_scs64_halo with 5 sixteenths resident, at the halo-fold worker's smallest brick: the worker's own checks (both
    solves equal the 2-rank restatement bit for bit, 7 / 5 launches per body)"""
    args = ["double", "fold", "scs", 64, 256, "hpcg16", 100]
    env = dict(os.environ, OMP_NUM_THREADS="1", SB_P2P="1", SB_P2P_REPORT="1", SB_SHARED_GPU="1")
    for k in ("SB_HALO_FOLD", "SB_HALO_PUSH_INSIDE", "SB_P2P_HALO", "SB_DOT_ORDER"):
        env.pop(k, None)
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(HERE, "gpu_resident_share_halo_worker.py")]
    out = subprocess.run(cmd + [str(a) for a in args], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=330)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-4000:]
    assert "HALO_FOLD_OK " + " ".join(str(a) for a in args) + " 2" in text, text[-3000:]
    assert text.count("RESIDENT_SHARE 5") == 2, text[-3000:]
    _need_peer_mapped_plane(text)
    _counts(text, 2, 0, 0, 7)
    _counts(text, 2, 1, 1, 5)
