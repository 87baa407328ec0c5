"""Case list and hand-made matrices of the SGS tests.  Matrices are named as pcg_cases names them:
("hpcg", n) | ("dims", nx, ny, nz) | ("scaled", n) | ("irregular", n) | ("file", path)."""
import os

import pcg_cases
from pcg_cases import BAND_KLEIN  # noqa: F401


def _c(matrix, fmt, C, sigma, itermax, eps_rel, **kw):
    return dict(matrix=matrix, fmt=fmt, C=C, sigma=sigma, itermax=itermax, eps_rel=eps_rel, **kw)


# the solves compared bit for bit on the GPU (tests/test_gpu_sgs.py) and pinned in tests/golden/sgs_hist.json
CASES = {
    "scaled16_crs": _c(("scaled", 16), "crs", 64, 1, 150, 1e-10),
    "scaled16_sell_64_1": _c(("scaled", 16), "scs", 64, 1, 150, 1e-10),
    "scaled16_sell_64_256": _c(("scaled", 16), "scs", 64, 256, 150, 1e-10),
    "hpcg16_sell_64_256": _c(("hpcg", 16), "scs", 64, 256, 60, 0.0),
    "dims_10_11_13_sell_64_256": _c(("dims", 10, 11, 13), "scs", 64, 256, 60, 0.0),
    "irregular12_crs": _c(("irregular", 12), "crs", 64, 1, 150, 1e-10),
    "irregular12_sell_64_256": _c(("irregular", 12), "scs", 64, 256, 150, 1e-10),
    "scaled8_sell_4_8": _c(("scaled", 8), "scs", 4, 8, 150, 1e-10),
    "hpcg64_sell_64_256": _c(("hpcg", 64), "scs", 64, 256, 60, 0.0, big=True),
}
SMALL = [n for n, c in CASES.items() if not c.get("big")]

# iteration counts to eps = 1e-10 ||b|| in the natural (CRS) order, Jacobi against SGS (golden: "counts")
COUNT_CASES = {
    "scaled16": _c(("scaled", 16), "crs", 64, 1, 150, 1e-10),
    "hpcg32": _c(("hpcg", 32), "crs", 64, 1, 150, 1e-10),
}
SCIPY_CASES = {
    "irregular12": _c(("irregular", 12), "crs", 64, 1, 150, 1e-10),
    "scaled16": _c(("scaled", 16), "crs", 64, 1, 150, 1e-10),
    "hpcg16": _c(("hpcg", 16), "crs", 64, 1, 150, 1e-10),
}

# the apply alone (tests/test_gpu_sgs_kernels.py): shapes x formats
KERNEL_SHAPES = [("dims", 5, 5, 5), ("dims", 7, 7, 6), ("dims", 33, 7, 5), ("dims", 17, 17, 17), ("dims", 19, 21, 23),
                 ("irregular", 12), ("file", BAND_KLEIN)]
KERNEL_FORMATS = [("crs", 64, 1), ("scs", 64, 1), ("scs", 64, 256)]


def write_mtx(path, n, entries):
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write("%d %d %d\n" % (n, n, len(entries)))
        f.write("".join("%d %d %.17g\n" % (r + 1, c + 1, v) for r, c, v in entries))
    return str(path)


def hand_made(kind, tmpdir):
    """path of a small matrix written into tmpdir: "one" 1 x 1 | "diagonal" 130 rows, nC = 1 | "arrow" 300 rows, row 0 coupled
    to all: nC = 2 | "zeros" a tridiagonal matrix of 70 rows plus stored explicit zeros off the diagonal (to be dropped)"""
    path = os.path.join(str(tmpdir), "sgs_%s.mtx" % kind)
    if kind == "one":
        ent = [(0, 0, 3.0)]
        n = 1
    elif kind == "diagonal":
        n = 130
        ent = [(i, i, float(pcg_cases.scale(i)) * 3.0) for i in range(n)]
    elif kind == "arrow":
        n = 300
        ent = [(0, 0, 400.0)] + [(0, j, -1.0 - (j % 3) * 0.25) for j in range(1, n)]
        for i in range(1, n):
            ent += [(i, 0, -1.0 - (i % 3) * 0.25), (i, i, 2.0 + (i % 5))]
    else:
        n = 70
        ent = []
        for i in range(n):
            if i > 0:
                ent.append((i, i - 1, -1.0))
            if i > 4:
                ent.append((i, i - 5, 0.0))  # stored, zero: no coupling, no colour
            ent.append((i, i, 4.0))
            if i < n - 1:
                ent.append((i, i + 1, -1.0))
            if i < n - 7:
                ent.append((i, i + 7, 0.0))
    return write_mtx(path, n, sorted(ent))
