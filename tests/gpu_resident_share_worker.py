"""The SpMV part of tests/test_gpu_resident_share.py: spmv_scs64 at every resident share against share 0 and the oracle, bit
for bit.  The test calls check_spmv() in its own process (XCD block mapping on) and starts this file once as a program with
SB_SCS_XCD=0 (the mapping is read once per process), where a block's position is its index in plain order."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import pyoracle as po  # noqa: E402
from sparsebench_amd.capi import DeviceVector  # noqa: E402

SHARES = (0, 1, 5, 8, 15, 16)
NAN = np.uint64(0x7FF8000000000000)


def bits(a):
    """the values' bit patterns, every NaN as one pattern (which payload an add of two NaNs returns is not the algorithm's)"""
    a = np.ascontiguousarray(a, np.float64)
    return np.where(np.isnan(a), NAN, a.view(np.uint64))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def ragged(rng, n, maxlen):
    """square, rows of 0 ... maxlen entries: chunks of very different widths, much padding at sigma 1"""
    lens = rng.integers(0, maxlen + 1, size=n)
    rp = np.zeros(n + 1, dtype=np.uint32)
    rp[1:] = np.cumsum(lens)
    col = rng.integers(0, n, size=int(rp[-1])).astype(np.uint32)
    return po.GMatrix.from_csr(rp, col, rng.standard_normal(int(rp[-1])), nc=n)


def matrices():
    rng = np.random.default_rng(7)
    return [("hpcg 4x4x4: 1 chunk", po.GMatrix.generate(4, 4, 4)),
            ("hpcg 8x8x5: 5 chunks, 2 blocks, the last partial", po.GMatrix.generate(8, 8, 5)),
            ("hpcg 16x16x9: 36 chunks, 9 blocks over 8 XCD ranges", po.GMatrix.generate(16, 16, 9)),
            ("ragged 1000 rows (not a multiple of 64)", ragged(rng, 1000, 40))]


def check_spmv(L):
    """returns how many (matrix, sigma, x, share) products were compared"""
    rng = np.random.default_rng(3)
    done = 0
    for name, g in matrices():
        for sigma in (1, 256):
            s = g.to_scs(64, sigma)
            arrs = [np.ascontiguousarray(a) for a in (s.chunkPtr, s.chunkLens, s.colInd, s.val, s.oldToNewPerm, s.newToOldPerm)]
            m = L.sb_scs_upload(s.nr, s.nc, s.C, s.sigma, s.nChunks, s.nElems, *[_p(a) for a in arrs])
            L.sb_matrix_use_packed(m, 0)  # the reference-layout kernel
            assert L.sb_matrix_packed_mode(m) == 0
            nq = 4 * ((s.nr + 255) // 256)
            for special in (False, True):
                x = rng.standard_normal(g.nc)
                if special:
                    x[0] = np.inf  # the padding terms 0.0 * x[0] become NaN: they must pass through both copies of the loop
                xp = x[np.asarray(s.newToOldPerm)] if L.sb_matrix_is_permuted(m) else x  # the device's row order
                y_ref = s.spmv_literal(x)[:s.nr]
                dx, dy = DeviceVector.from_host(xp), DeviceVector(s.nr)
                first = None
                for k in SHARES:
                    what = (name, sigma, special, k)
                    assert L.sb_matrix_resident_share(m, k) == k, what
                    dy.set(np.full(s.nr, 7.0))
                    dq = DeviceVector.from_host(np.full(nq, 7.0))
                    assert L.sb_spmv_native_dot(m, dx.ptr, dy.ptr, dq.ptr) == 2, what
                    y, q = dy.get(), dq.get()
                    dq.free()
                    assert np.array_equal(bits(y), bits(y_ref)), ("y vs the oracle",) + what
                    assert np.array_equal(bits(q[:nq // 4]), bits(po.ddot_partials(xp[:s.nr].copy(), y))), ("level-1 dot vs the oracle",) + what
                    if first is None:
                        first = (y, q[:nq // 4])
                    assert np.array_equal(bits(y), bits(first[0])) and np.array_equal(bits(q[:nq // 4]), bits(first[1])), ("vs share 0",) + what
                    if special and name.startswith("ragged") and sigma == 1:
                        assert np.isnan(y).any(), what  # (rows shorter than their chunk: the padding terms were taken)
                    # the plain product (no fused dot) is the other instantiation of the kernel
                    dy.set(np.full(s.nr, 7.0))
                    L.sb_spmv_native(m, dx.ptr, dy.ptr)
                    assert np.array_equal(bits(dy.get()), bits(y_ref)), ("plain product",) + what
                    done += 1
                dx.free(), dy.free()
            L.sb_matrix_free(m)
    return done


if __name__ == "__main__":
    from sparsebench_amd import capi
    assert os.environ.get("SB_SCS_XCD") == "0"
    print("RESIDENT_SHARE_SPMV_OK xcd=0 products=%d" % check_spmv(capi.init(0)), flush=True)
