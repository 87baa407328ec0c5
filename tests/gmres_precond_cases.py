"""Case list of the tests of right-preconditioned GMRES(m): the matrices, formats and plans of
bicgstab_precond_cases crossed with the restart length m, and the diagonals.  Every case runs to eps = 1e-10 ||b|| at itermax 150.

precond: "none" | "jacobi" | "signed" (the caller's diagonal, entries of both signs) | "sgs" | "poly" | "mgpoly" as
bicgstab_precond_cases names them; `aggregation`: the mgpoly hierarchy is aggregation_ref's (theta = 0, omega_s = 4/3, omega = 1);
`device_product`: the coarse matrix is the device's product of a FILE matrix, which only a GPU test can form (the CPU tests and the
golden file leave the case out).  TEST INFRASTRUCTURE ONLY.
"""
import numpy as np

import bicgstab_precond_cases as bc
from bicgstab_cases import CD16, SCD16
from pcg_cases import scale

S256 = bc.S256
CD32 = ("cd", 32, 32, 32)


def signed_scale(idx):
    """the caller's diagonal of the "signed" cases, original row order: 2^((i mod 7) - 3) over the diagonal's 6, every fifth
    entry negative.  Finite and non-zero, not positive: what a PCG handle refuses and GMRES takes"""
    idx = np.asarray(idx)
    return scale(idx) / 6.0 * np.where(idx % 5 == 4, -1.0, 1.0)


def _with_m(name, m, **kw):
    return dict(bc.CASES[name], m=m, **kw)


def _diag(matrix, f, precond, m):
    return dict(matrix=matrix, fmt=f[0], C=f[1], sigma=f[2], precond=precond, itermax=150, eps_rel=1e-10, m=m)


CASES = {}
for _f in bc.FORMATS:
    for _p in ("sgs", "poly_3_16", "poly_1_16"):
        CASES["cd16_%s_%s_m30" % (_f, _p)] = _with_m("cd16_%s_%s" % (_f, _p), 30)
CASES.update({
    "cd16_sell_64_256_poly_3_16_m10": _with_m("cd16_sell_64_256_poly_3_16", 10),
    "cd16_sell_64_256_poly_3_16_m1": _with_m("cd16_sell_64_256_poly_3_16", 1),  # every step closes: the close's rider each step
    "cd_10_11_13_sell_64_256_poly_3_16_m30": _with_m("cd_10_11_13_sell_64_256_poly_3_16", 30),
    "cd_10_11_13_sell_64_256_poly_3_16_m1": _with_m("cd_10_11_13_sell_64_256_poly_3_16", 1),
    "scaled_cd16_sell_64_256_jacobi_m30": _diag(SCD16, S256, "jacobi", 30),
    "scaled_cd16_sell_64_256_poly_3_16_m30": _with_m("scaled_cd16_sell_64_256_poly_3_16", 30),
    "cd16_sell_64_256_signed_m30": _diag(CD16, S256, "signed", 30),
    "hpcg16_sell_64_256_mgpoly_regenerated_m30": _with_m("hpcg16_sell_64_256_mgpoly_regenerated", 30),
    "hpcg16_sell_64_256_mgpoly_galerkin_m30": _with_m("hpcg16_sell_64_256_mgpoly_galerkin", 30),
    "cd16_sell_64_256_mgpoly_2_levels_1_step_m30": _with_m("cd16_sell_64_256_mgpoly_2_levels_1_step", 30),
    "cd16_sell_64_256_mgpoly_aggregation_m30": dict(matrix=CD16, fmt="scs", C=64, sigma=256, precond="mgpoly", steps=1,
                                                    aggregation=True, itermax=150, eps_rel=1e-10, m=30),
    "cd32_sell_64_256_poly_3_16_m30": _with_m("cd32_sell_64_256_poly_3_16", 30),
})
HOST_CASES = {name: c for name, c in CASES.items() if not c.get("device_product")}
# the cases whose solve reaches eps inside itermax.  The signed diagonal makes A D indefinite: it is there for the bits of a
# diagonal with negative entries, not for its iteration count
CONVERGING = [name for name in HOST_CASES if HOST_CASES[name]["precond"] != "signed"]

# k to eps = 1e-10 ||b|| in CRS at itermax 400 (DESIGN 4.20's table).  (matrix, m) -> column -> k; the columns: "none", "jacobi",
# "sgs", "poly" (3, 16), "mgpoly": one step, scipy's P^T A P, omega = 1, ratio 4, the automatic depth
CRS = bc.CRS
HPCG16 = ("hpcg", 16)
COLUMNS = ("none", "jacobi", "sgs", "poly", "mgpoly")
TABLE = {
    (CD16, 30): {"none": 112, "jacobi": 112, "sgs": 31, "poly": 27, "mgpoly": 22},
    (CD16, 10): {"none": 111, "jacobi": 111, "sgs": 62, "poly": 44, "mgpoly": 24},
    (SCD16, 30): {"none": 265, "jacobi": 112, "sgs": 31, "poly": 54, "mgpoly": 46},
    (SCD16, 10): {"none": 209, "jacobi": 111, "sgs": 62, "poly": 82, "mgpoly": 48},
    (HPCG16, 30): {"none": 27, "jacobi": 27, "sgs": 21, "poly": 16, "mgpoly": 9},
    (HPCG16, 10): {"none": 48, "jacobi": 48, "sgs": 23, "poly": 16, "mgpoly": 9},
}


def table_case(matrix, m, column):
    f = CRS
    if column in ("none", "jacobi"):
        return dict(_diag(matrix, f, column, m), itermax=400)
    if column == "sgs":
        return dict(bc._c(matrix, *f, "sgs"), m=m, itermax=400)
    if column == "poly":
        return dict(bc._c(matrix, *f, "poly", steps=3, ratio=16.0), m=m, itermax=400)
    return dict(bc._c(matrix, *f, "mgpoly", steps=1, levels=None, ratio=4.0, galerkin=True), m=m, itermax=400)
