"""The odd HPCG shapes of the single-precision loop tests (tests/test_gpu_sp_odd_shapes.py) and their CPU restatement on
tests/sp_ref.py, for the tests only.  Row counts off the 4 / 64 / 256 grids: the last float4 of the loop kernels is partial, the
last 256-group of the tree dot is ragged, and at 266 175 rows level 2 of the tree makes a second trip over its 1024 threads.

shape -> (itermax, rows, level-1 values)"""
import numpy as np

import sp_ref
from sparsebench_amd import hostapi

F = np.float32
SHAPES = {
    (5, 5, 5): (60, 125, 1),           # n % 4 = 1, n < 256: one partial group
    (7, 7, 6): (60, 294, 2),           # n % 4 = 2, just over one group
    (33, 7, 5): (60, 1155, 5),         # n % 4 = 3, the fp64 loop's own odd shape
    (17, 17, 17): (60, 4913, 20),      # n % 4 = 1, two p-update workgroups, two r-update workgroups
    (19, 21, 23): (40, 9177, 36),      # n % 4 = 1, seq dot: a second LDS block of 985 elements (985 % 16 = 9)
    (65, 65, 63): (12, 266175, 1040),  # n % 4 = 3, level 2's second trip for 16 threads; tree order only
}
BIG = (65, 65, 63)
# the mirror's probes (whether a mirror is built is known on the device only): 16 512 rows (n % 256 = 128) and 6 336 rows
MIRROR_SHAPES = {(128, 43, 3): 40, (64, 33, 3): 40}


def bits(a):
    a = np.asarray(a, F)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def same_bits(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def equal_runs(a, b):
    """(k, r.r history, p.Ap history, x) bit for bit"""
    return a[0] == b[0] and all(same_bits(u, v) for u, v in zip(a[1:], b[1:]))


class Restatement:
    """sp_ref.cg over sp_ref.spmv_crs at one shape; each history computed once and kept"""

    def __init__(self, shape, itermax):
        c = hostapi.Problem("generate", shape[0], shape[1], shape[2], fmt="crs", upload=False, precision="single")
        self.rp, self.col, self.val = c.array("rowPtr").copy(), c.array("crs_colInd").copy(), c.values().copy()
        self.b = c.rhs()[0].copy()
        self.nr = c.nr
        c.free()
        self.itermax = itermax
        self.kept = {}

    def _cg(self, spmv, b, dot):
        with np.errstate(all="ignore"):
            return sp_ref.cg(spmv, b, self.itermax, dot=dot)

    def seq(self):
        """the seq order runs over the caller's row order in every format"""
        if "seq" not in self.kept:
            self.kept["seq"] = self._cg(lambda v: sp_ref.spmv_crs(self.rp, self.col, self.val, v), self.b, sp_ref.dot_seq)
        return self.kept["seq"]

    def tree(self, oldToNew=None):
        """the tree runs over the device's row order: the caller's, or (oldToNew: a Sell-C-sigma matrix with sigma > 1) the
        permuted one -- CG on P A P^T and P b, x carried back"""
        if oldToNew is None or np.array_equal(oldToNew, np.arange(self.nr)):
            if "tree" not in self.kept:
                self.kept["tree"] = self._cg(lambda v: sp_ref.spmv_crs(self.rp, self.col, self.val, v), self.b, sp_ref.dot_tree)
            return self.kept["tree"]
        o2n = np.asarray(oldToNew, np.int64)
        key = ("tree", o2n.tobytes())
        if key not in self.kept:
            n2o = np.empty(self.nr, np.int64)
            n2o[o2n] = np.arange(self.nr)
            k, rr, pap, xd = self._cg(lambda vd: sp_ref.spmv_crs(self.rp, self.col, self.val, vd[o2n])[n2o], self.b[n2o], sp_ref.dot_tree)
            self.kept[key] = (k, rr, pap, xd[o2n])
        return self.kept[key]
