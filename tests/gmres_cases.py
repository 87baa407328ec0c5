"""Test matrices and case list of the GMRES tests.

`write_convdiff` writes a NON-symmetric matrix as a `general` Matrix Market file: 7-point upwind convection-diffusion on an
nx x ny x nz grid, diagonal 6, the three lower neighbours -1.5, the three upper neighbours -0.5 -- every value exact in
binary; b = 1 by the file rule of initVectors.  CG cannot solve it; GMRES can.
"""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND_KLEIN = os.path.join(ROOT, "tests", "golden", "ref", "matrix_band_klein.mtx")


def convdiff_entries(nx, ny, nz):
    """rows of (row, col, val), 0-based, ordered by row then column"""
    out = []
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                r = (z * ny + y) * nx + x
                if z > 0:
                    out.append((r, r - nx * ny, -1.5))
                if y > 0:
                    out.append((r, r - nx, -1.5))
                if x > 0:
                    out.append((r, r - 1, -1.5))
                out.append((r, r, 6.0))
                if x < nx - 1:
                    out.append((r, r + 1, -0.5))
                if y < ny - 1:
                    out.append((r, r + nx, -0.5))
                if z < nz - 1:
                    out.append((r, r + nx * ny, -0.5))
    return out


def write_convdiff(path, nx, ny, nz):
    ent = convdiff_entries(nx, ny, nz)
    n = nx * ny * nz
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write("%d %d %d\n" % (n, n, len(ent)))
        for r, c, v in ent:
            f.write("%d %d %.1f\n" % (r + 1, c + 1, v))
    return str(path)


# name -> what to build and how to solve it.  kind "cd": convection-diffusion dims; "hpcg": the generated 27-point stencil in
# Sell-64-256's permuted row order; "file": a Matrix Market file of the repository.  eps_rel: eps = eps_rel * ||b||.
CASES = {
    "cd16_m30": dict(kind="cd", dims=(16, 16, 16), m=30, itermax=150, eps_rel=1e-10),
    "cd16_m10": dict(kind="cd", dims=(16, 16, 16), m=10, itermax=150, eps_rel=1e-10),
    "cd16_m1": dict(kind="cd", dims=(16, 16, 16), m=1, itermax=150, eps_rel=1e-10),
    "cd_10_11_13_m30": dict(kind="cd", dims=(10, 11, 13), m=30, itermax=150, eps_rel=1e-10),
    "cd32_m30": dict(kind="cd", dims=(32, 32, 32), m=30, itermax=150, eps_rel=1e-10),
    "hpcg16_m30": dict(kind="hpcg", dims=(16, 16, 16), m=30, itermax=60, eps_rel=0.0),
    "hpcg32_m30": dict(kind="hpcg", dims=(32, 32, 32), m=30, itermax=60, eps_rel=0.0),
    "band_klein_eps": dict(kind="file", path=BAND_KLEIN, m=30, itermax=150, eps_rel=1e-10),
    "band_klein_eps0": dict(kind="file", path=BAND_KLEIN, m=30, itermax=21, eps_rel=0.0),
    "hpcg64_m30": dict(kind="hpcg", dims=(64, 64, 64), m=30, itermax=150, eps_rel=0.0, big=True),
    "hpcg128_m30": dict(kind="hpcg", dims=(128, 128, 128), m=30, itermax=60, eps_rel=0.0, big=True),
}
SCIPY_CASES = ("cd16_m30", "cd16_m10", "cd_10_11_13_m30", "cd16_m1")
