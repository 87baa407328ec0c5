"""Worker of tests/test_gpu_resident_share.py: tests/gpu_halo_fold_worker.py as it is, with a resident share of 5 sixteenths
forced on every rank's matrix where that worker selects the reference-layout kernel -- so that spmv_scs64_halo runs with both
kinds of block and must still give the P-rank restatement's bits (ranks that share a device get share 0 from the rule)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_halo_fold_worker as worker  # noqa: E402
from sparsebench_amd import hostapi  # noqa: E402

_use_packed = hostapi.Problem.use_packed


def use_packed(self, mode):
    got = _use_packed(self, mode)
    assert self.resident_share(-1) == 0, "ranks share the device: the rule must give share 0"
    assert self.resident_share(5) == 5
    print("RESIDENT_SHARE 5", flush=True)
    return got


hostapi.Problem.use_packed = use_packed
worker.main()
