"""Case list and hand-made hierarchies of the MG tests.  Matrices are named as pcg_cases names them; a case has
`levels` (the geometric hierarchy of a generated matrix at that depth) or `coarse`: [(matrix, f2c), ...] with f2c an array or
("geo", nx, ny, nz), the geometric injection map of that grid."""
import os

import numpy as np

import sgs_cases


def _c(matrix, fmt, C, sigma, itermax, eps_rel, **kw):
    return dict(matrix=matrix, fmt=fmt, C=C, sigma=sigma, itermax=itermax, eps_rel=eps_rel, **kw)


# the solves compared bit for bit on the GPU (tests/test_gpu_mg.py) and pinned in tests/golden/mg_hist.json
CASES = {
    "hpcg16_sell_64_256_L4": _c(("hpcg", 16), "scs", 64, 256, 60, 0.0, levels=4),
    "hpcg16_crs_L3": _c(("hpcg", 16), "crs", 64, 1, 150, 1e-10, levels=3),
    "hpcg16_crs_L4": _c(("hpcg", 16), "crs", 64, 1, 150, 1e-10, levels=4),
    # the drivers' cases in a permuted order (-s 256), where the coarse levels change the iterates (test_gpu_mg_driver.py)
    "hpcg16_sell_64_256_L3_i20": _c(("hpcg", 16), "scs", 64, 256, 20, 0.0, levels=3),
    "hpcg16_sell_64_256_L4_i20": _c(("hpcg", 16), "scs", 64, 256, 20, 0.0, levels=4),
    "dims_12_8_20_sell_64_256_L3": _c(("dims", 12, 8, 20), "scs", 64, 256, 60, 0.0, levels=3),
    # a file matrix (the scaled stencil at 16^3) over a caller-supplied coarse level, the plain stencil at 8^3
    "scaled16_sell_64_256_over_hpcg8": _c(("scaled", 16), "scs", 64, 256, 150, 1e-10, coarse=[(("hpcg", 8), ("geo", 16, 16, 16))]),
    "hpcg64_sell_64_256_L4": _c(("hpcg", 64), "scs", 64, 256, 60, 0.0, levels=4, big=True),
}
SMALL = [n for n, c in CASES.items() if not c.get("big")]

# iteration counts to eps = 1e-10 ||b||: Jacobi, SGS, the two sweeps of MG's level 0 without its coarse levels, MG at auto
# depth; in the natural (CRS) order and in a permuted one (golden: "counts")
COUNT_CASES = {
    "hpcg16": _c(("hpcg", 16), "crs", 64, 1, 150, 1e-10, levels=None),
    "hpcg32": _c(("hpcg", 32), "crs", 64, 1, 150, 1e-10, levels=None),
    "hpcg16_sell_64_256": _c(("hpcg", 16), "scs", 64, 256, 150, 1e-10, levels=None),
    "hpcg32_sell_64_256": _c(("hpcg", 32), "scs", 64, 256, 150, 1e-10, levels=None),
}
# one V-cycle and whole solves against an independent scipy formulation (golden: "scipy_gap")
SCIPY_CASES = {
    "hpcg8_L2": _c(("hpcg", 8), "crs", 64, 1, 150, 1e-10, levels=2),
    "hpcg16_L4": _c(("hpcg", 16), "crs", 64, 1, 150, 1e-10, levels=4),
    "dims_12_8_20_L3": _c(("dims", 12, 8, 20), "crs", 64, 1, 150, 1e-10, levels=3),
    "scaled16_over_hpcg8": _c(("scaled", 16), "crs", 64, 1, 150, 1e-10, coarse=[(("hpcg", 8), ("geo", 16, 16, 16))]),
}

# the apply alone (tests/test_gpu_mg_kernels.py): shapes x formats.  4^3: the coarse level has 8 rows, one partial chunk of the
# restriction; 16^3 at HPCG's depth; 12 x 8 x 20: odd coarse dimensions, so the coarse colouring is not the parity one;
# 34 x 6 x 10: every colour of the fine level ends in a partial chunk
KERNEL_SHAPES = [(("dims", 4, 4, 4), 2), (("dims", 8, 8, 8), 3), (("dims", 16, 16, 16), 4), (("dims", 12, 8, 20), 3),
                 (("dims", 34, 6, 10), 2)]
KERNEL_FORMATS = [("crs", 64, 1), ("scs", 64, 1), ("scs", 64, 256)]
SELL_4_8_SHAPE = (("dims", 8, 8, 8), 3)


def tridiagonal(path, n, diag):
    ent = []
    for i in range(n):
        if i > 0:
            ent.append((i, i - 1, -1.0))
        ent.append((i, i, diag + (i % 3) * 0.5))
        if i < n - 1:
            ent.append((i, i + 1, -1.0))
    return sgs_cases.write_mtx(path, n, ent)


def hand_made(tmpdir):
    """a caller's hierarchy on files: a tridiagonal matrix of 130 rows, its even rows as the coarse points, a tridiagonal
    matrix of 65 rows on them: one full chunk of the restriction plus one lane.  Returns (fine path, coarse path, f2c)"""
    fine = tridiagonal(os.path.join(str(tmpdir), "mg_tri_130.mtx"), 130, 4.0)
    coarse = tridiagonal(os.path.join(str(tmpdir), "mg_tri_65.mtx"), 65, 3.0)
    return fine, coarse, np.arange(0, 130, 2)
