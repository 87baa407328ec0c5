"""Test matrices and case list of the PCG tests.

`write_scaled_hpcg` writes S A S as a `general` Matrix Market file: A the generated 27-point stencil of an n x n x n grid, S
diagonal with s_i = 2^((i mod 7) - 3).  Every value is a power of two times a stencil value, exact in binary and written with
%.17g; b = 1 by the file rule of initVectors.  The scaling spreads the diagonal over 2^-6 .. 2^6 times the stencil's: plain CG
crawls on it, Jacobi undoes it.
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND_KLEIN = os.path.join(ROOT, "tests", "golden", "ref", "matrix_band_klein.mtx")


def scale(i):
    """s_i = 2^((i mod 7) - 3); also the caller-supplied dinv of the tests"""
    return 2.0 ** ((np.asarray(i, dtype=np.int64) % 7) - 3)


def write_scaled_hpcg(path, n):
    from oracle import pyoracle as po
    g = po.GMatrix.generate(n, n, n)
    rp, col, val = g.rowPtr.astype(np.int64), g.col.astype(np.int64), g.val.copy()
    row = np.repeat(np.arange(g.nr, dtype=np.int64), np.diff(rp))
    v = (scale(row) * val) * scale(col)  # powers of two: both products exact
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write("%d %d %d\n" % (g.nr, g.nr, len(v)))
        f.write("".join("%d %d %.17g\n" % (r + 1, c + 1, x) for r, c, x in zip(row.tolist(), col.tolist(), v.tolist())))
    g.free()
    return str(path)


# name -> matrix, format and solve.  matrix: ("hpcg", n) | ("dims", nx, ny, nz) | ("scaled", n) | ("irregular", n) | ("file", path);
# dinv: "jacobi" | "identity" | "scale" (dinv_i = 2^((i mod 7) - 3), original row order); eps_rel: eps = eps_rel * ||b||
def _c(matrix, fmt, C, sigma, dinv, itermax, eps_rel, **kw):
    return dict(matrix=matrix, fmt=fmt, C=C, sigma=sigma, dinv=dinv, itermax=itermax, eps_rel=eps_rel, **kw)


CASES = {
    "irregular12_crs": _c(("irregular", 12), "crs", 64, 1, "jacobi", 150, 1e-10),
    "irregular12_sell_64_256": _c(("irregular", 12), "scs", 64, 256, "jacobi", 150, 1e-10),
    "scaled16_crs": _c(("scaled", 16), "crs", 64, 1, "jacobi", 150, 1e-10),
    "scaled16_sell_64_1": _c(("scaled", 16), "scs", 64, 1, "jacobi", 150, 1e-10),
    "scaled16_sell_64_256": _c(("scaled", 16), "scs", 64, 256, "jacobi", 150, 1e-10),
    "scaled8_sell_4_8": _c(("scaled", 8), "scs", 4, 8, "jacobi", 150, 1e-10),
    "dims_10_11_13_sell_64_256": _c(("dims", 10, 11, 13), "scs", 64, 256, "jacobi", 60, 0.0),
    "hpcg16_sell_64_256": _c(("hpcg", 16), "scs", 64, 256, "jacobi", 60, 0.0),
    "hpcg32_sell_64_256": _c(("hpcg", 32), "scs", 64, 256, "jacobi", 60, 0.0),
    "hpcg16_scale_sell_64_256": _c(("hpcg", 16), "scs", 64, 256, "scale", 60, 0.0),
    "hpcg64_scale_sell_64_256": _c(("hpcg", 64), "scs", 64, 256, "scale", 60, 0.0, big=True),
    "hpcg128_sell_64_256": _c(("hpcg", 128), "scs", 64, 256, "jacobi", 60, 0.0, big=True),
}
SMALL = [n for n, c in CASES.items() if not c.get("big")]
# against scipy's preconditioned CG (name -> the case solved with eps = 1e-10 ||b||)
SCIPY_CASES = {
    "irregular12": _c(("irregular", 12), "crs", 64, 1, "jacobi", 150, 1e-10),
    "scaled16": _c(("scaled", 16), "crs", 64, 1, "jacobi", 150, 1e-10),
    "hpcg16": _c(("hpcg", 16), "crs", 64, 1, "jacobi", 150, 1e-10),
}
