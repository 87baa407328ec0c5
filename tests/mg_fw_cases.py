"""Case list and the hand-made hierarchy of the tests of the V-cycle with full-weighting transfers.  Matrices are
named as pcg_cases names them; a case has `levels` (the geometric hierarchy of a generated matrix at that depth with the
trilinear P and omega = 0.5) or `coarse`: [(matrix, P, omega), ...] with P a (ptr, col, val) triple or ("tri", nx, ny, nz), the
trilinear prolongation onto that grid."""
import numpy as np

import mg_cases
from mg_cases import KERNEL_SHAPES, KERNEL_FORMATS, SELL_4_8_SHAPE, COUNT_CASES  # noqa: F401  (the same shapes and count cases)


def _c(matrix, fmt, C, sigma, itermax, eps_rel, **kw):
    return dict(matrix=matrix, fmt=fmt, C=C, sigma=sigma, itermax=itermax, eps_rel=eps_rel, **kw)


# the solves compared bit for bit on the GPU (tests/test_gpu_mg_fw.py) and pinned in tests/golden/mg_fw_hist.json: the twins of
# mg_cases.SMALL, and one big case at 32^3
CASES = {
    "hpcg16_crs_L3": _c(("hpcg", 16), "crs", 64, 1, 150, 1e-10, levels=3),
    "hpcg16_crs_L4": _c(("hpcg", 16), "crs", 64, 1, 150, 1e-10, levels=4),
    "hpcg16_sell_64_256_L4": _c(("hpcg", 16), "scs", 64, 256, 150, 1e-10, levels=4),
    # the driver's -l 3 case in a permuted order (test_gpu_mg_fw_driver.py)
    "hpcg16_sell_64_256_L3": _c(("hpcg", 16), "scs", 64, 256, 150, 1e-10, levels=3),
    "dims_12_8_20_sell_64_256_L3": _c(("dims", 12, 8, 20), "scs", 64, 256, 150, 1e-10, levels=3),
    # a file matrix (the scaled stencil at 16^3) over a caller-supplied coarse level, the plain stencil at 8^3, trilinear P
    "scaled16_sell_64_256_over_hpcg8": _c(("scaled", 16), "scs", 64, 256, 150, 1e-10,
                                          coarse=[(("hpcg", 8), ("tri", 16, 16, 16), 0.5)]),
    "hpcg32_sell_64_256_L4": _c(("hpcg", 32), "scs", 64, 256, 150, 1e-10, levels=4, big=True),
}
SMALL = [n for n, c in CASES.items() if not c.get("big")]

# one V-cycle and whole solves against an independent scipy formulation (golden: "scipy_gap"): mg_cases.SCIPY_CASES' twins
SCIPY_CASES = {
    "hpcg8_L2": _c(("hpcg", 8), "crs", 64, 1, 150, 1e-10, levels=2),
    "hpcg16_L4": _c(("hpcg", 16), "crs", 64, 1, 150, 1e-10, levels=4),
    "dims_12_8_20_L3": _c(("dims", 12, 8, 20), "crs", 64, 1, 150, 1e-10, levels=3),
    "scaled16_over_hpcg8": _c(("scaled", 16), "crs", 64, 1, 150, 1e-10, coarse=[(("hpcg", 8), ("tri", 16, 16, 16), 0.5)]),
}
TRILINEAR_DIMS = [(4, 4, 4), (8, 8, 8), (12, 8, 20), (34, 6, 10)]

EMPTY_ROW, ZERO_WEIGHT_ROW = 7, 21  # of the hand-made P below


def linear_1d(n, empty_row=EMPTY_ROW, zero_weight_row=ZERO_WEIGHT_ROW, store_zero=True):
    """1-D linear interpolation from n // 2 + n % 2 points (the even rows) onto n: even row i takes i / 2 with weight 1, odd row i
    (i - 1) / 2 and (i + 1) / 2 with 1/2 each.  Row `empty_row` is left without an entry; the second weight of row
    `zero_weight_row` is a stored 0.0 (store_zero False: left out, which must change nothing)"""
    nc = (n + 1) // 2
    ptr, col, val = [0], [], []
    for i in range(n):
        if i != empty_row:
            if i % 2 == 0:
                col.append(i // 2), val.append(1.0)
            else:
                col.append((i - 1) // 2), val.append(0.5)
                if (i + 1) // 2 < nc:
                    if i != zero_weight_row:
                        col.append((i + 1) // 2), val.append(0.5)
                    elif store_zero:
                        col.append((i + 1) // 2), val.append(0.0)
        ptr.append(len(col))
    return np.array(ptr, dtype=np.int64), np.array(col, dtype=np.int64), np.array(val)


def hand_made(tmpdir, store_zero=True):
    """a caller's hierarchy on files: mg_cases.hand_made's tridiagonal matrices of 130 and 65 rows with 1-D linear interpolation
    as P, one row of it empty, one stored weight 0.0, omega = 0.5.  Returns (fine path, coarse path, P, omega)"""
    assert EMPTY_ROW % 2 == 1 and ZERO_WEIGHT_ROW % 2 == 1
    fine, coarse, _ = mg_cases.hand_made(tmpdir)
    return fine, coarse, linear_1d(130, store_zero=store_zero), 0.5


def hand_made_case(tmpdir, fmt="crs", sigma=1, store_zero=True):
    fine, coarse, P, omega = hand_made(tmpdir, store_zero)
    return dict(matrix=("file", fine), fmt=fmt, C=64, sigma=sigma, itermax=150, eps_rel=1e-10, coarse=[(("file", coarse), P, omega)])
