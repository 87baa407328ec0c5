"""Test matrices and case list of the BiCGStab tests.

The non-symmetric matrix is the upwind convection-diffusion of gmres_cases (`write_convdiff`).  `write_scaled_convdiff` writes
A S of it as a `general` Matrix Market file: S diagonal with s_i = 2^((i mod 7) - 3) (`pcg_cases.scale`), so column j of A is
multiplied by a power of two.  Every value is exact in binary and written with %.17g; b = 1 by the file rule of initVectors.
The scaling spreads the diagonal over 2^-3 .. 2^3 times 6: unpreconditioned BiCGStab needs about twice the bodies, the Jacobi
right preconditioner undoes it (1 / d_i = 1 / (6 s_i)).  The caller's dinv = s of the case list is a diagonal that is NOT the
Jacobi one (it makes A S^2 of it): it is there for the bits, not for the iteration count.
"""
import os

import numpy as np

from gmres_cases import convdiff_entries, write_convdiff  # noqa: F401  (write_convdiff: re-exported for the tests)
from pcg_cases import scale  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_scaled_convdiff(path, nx, ny, nz):
    ent = convdiff_entries(nx, ny, nz)
    n = nx * ny * nz
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write("%d %d %d\n" % (n, n, len(ent)))
        f.write("".join("%d %d %.17g\n" % (r + 1, c + 1, v * float(scale(c))) for r, c, v in ent))  # power of two: exact
    return str(path)


# name -> matrix, format and solve.  matrix: ("cd", nx, ny, nz) | ("scaled_cd", nx, ny, nz) | ("hpcg", n) | ("dims", nx, ny, nz);
# precond: "none" | "jacobi" | "scale" (the caller's dinv_i = 2^((i mod 7) - 3), original row order); eps = eps_rel * ||b||
def _c(matrix, fmt, C, sigma, precond, itermax, eps_rel):
    return dict(matrix=matrix, fmt=fmt, C=C, sigma=sigma, precond=precond, itermax=itermax, eps_rel=eps_rel)


CD16 = ("cd", 16, 16, 16)
SCD16 = ("scaled_cd", 16, 16, 16)
CASES = {
    "cd16_crs_none": _c(CD16, "crs", 64, 1, "none", 150, 1e-10),
    "cd16_crs_jacobi": _c(CD16, "crs", 64, 1, "jacobi", 150, 1e-10),
    "cd16_sell_64_1_none": _c(CD16, "scs", 64, 1, "none", 150, 1e-10),
    "cd16_sell_64_1_jacobi": _c(CD16, "scs", 64, 1, "jacobi", 150, 1e-10),
    "cd16_sell_64_256_none": _c(CD16, "scs", 64, 256, "none", 150, 1e-10),
    "cd16_sell_64_256_jacobi": _c(CD16, "scs", 64, 256, "jacobi", 150, 1e-10),
    "cd16_sell_4_8_none": _c(CD16, "scs", 4, 8, "none", 150, 1e-10),
    "cd16_sell_4_8_jacobi": _c(CD16, "scs", 4, 8, "jacobi", 150, 1e-10),
    "cd_10_11_13_sell_64_256_none": _c(("cd", 10, 11, 13), "scs", 64, 256, "none", 150, 1e-10),
    "cd_5_3_2_crs_none": _c(("cd", 5, 3, 2), "crs", 64, 1, "none", 150, 1e-10),
    "scaled_cd16_sell_64_256_jacobi": _c(SCD16, "scs", 64, 256, "jacobi", 150, 1e-10),
    "scaled_cd16_sell_64_256_scale": _c(SCD16, "scs", 64, 256, "scale", 150, 1e-10),
    "hpcg16_sell_64_256_none": _c(("hpcg", 16), "scs", 64, 256, "none", 60, 0.0),
    "hpcg32_sell_64_256_none": _c(("hpcg", 32), "scs", 64, 256, "none", 60, 0.0),
    "dims_64_64_72_sell_64_256_none": _c(("dims", 64, 64, 72), "scs", 64, 256, "none", 40, 0.0),
}
# the restatement on the CPU (tests/test_bicgstab_host.py): eps = 1e-10 ||b||, itermax 150
HOST_CASES = {
    "cd16": _c(CD16, "crs", 64, 1, "none", 150, 1e-10),
    "cd_10_11_13": _c(("cd", 10, 11, 13), "crs", 64, 1, "none", 150, 1e-10),
    "cd_5_3_2": _c(("cd", 5, 3, 2), "crs", 64, 1, "none", 150, 1e-10),
    "scaled_cd16_none": _c(SCD16, "crs", 64, 1, "none", 150, 1e-10),
    "scaled_cd16_jacobi": _c(SCD16, "crs", 64, 1, "jacobi", 150, 1e-10),
    "hpcg16": _c(("hpcg", 16), "scs", 64, 256, "none", 150, 1e-10),
}
