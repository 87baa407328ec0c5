"""Case list of the tests of BiCGStab under a preconditioner plan.  The matrices are bicgstab_cases' (the upwind
convection-diffusion `cd`, its column-scaled form `scaled_cd`) and the generated 27-point stencil; every case runs to
eps = 1e-10 ||b|| at itermax 150.

precond: "sgs" | "poly" (steps, ratio) | "mgpoly" (steps; `levels`: None is the deepest of up to 4; `galerkin`: False -- the
stencil regenerated on every halved grid, omega = 0.25 -- or "device": A_{l+1} = P_l^T A_l P_l with the trilinear P, omega = 1).
`device_product`: the coarse matrices are the device's product of a FILE matrix, which only a GPU test can form: the test hands
the downloaded product to the restatement, and the CPU tests and the golden file leave the case out.
"""
from bicgstab_cases import CD16, SCD16


def _c(matrix, fmt, C, sigma, precond, **kw):
    return dict(dict(matrix=matrix, fmt=fmt, C=C, sigma=sigma, precond=precond, itermax=150, eps_rel=1e-10), **kw)


FORMATS = {"crs": ("crs", 64, 1), "sell_64_1": ("scs", 64, 1), "sell_64_256": ("scs", 64, 256), "sell_4_8": ("scs", 4, 8)}
S256 = FORMATS["sell_64_256"]

CASES = {}
for _name, _f in FORMATS.items():
    CASES["cd16_%s_sgs" % _name] = _c(CD16, *_f, "sgs")
    CASES["cd16_%s_poly_3_16" % _name] = _c(CD16, *_f, "poly", steps=3, ratio=16.0)
    CASES["cd16_%s_poly_1_16" % _name] = _c(CD16, *_f, "poly", steps=1, ratio=16.0)
CASES.update({
    "scaled_cd16_sell_64_256_sgs": _c(SCD16, *S256, "sgs"),
    "scaled_cd16_sell_64_256_poly_3_16": _c(SCD16, *S256, "poly", steps=3, ratio=16.0),
    "cd_10_11_13_sell_64_256_poly_3_16": _c(("cd", 10, 11, 13), *S256, "poly", steps=3, ratio=16.0),
    "cd16_sell_64_256_mgpoly_2_levels_1_step": _c(CD16, *S256, "mgpoly", steps=1, levels=2, ratio=4.0, galerkin="device",
                                                  device_product=True),
    "hpcg16_sell_64_256_mgpoly_regenerated": _c(("hpcg", 16), *S256, "mgpoly", steps=1, levels=None, ratio=4.0, galerkin=False),
    "hpcg16_sell_64_256_mgpoly_galerkin": _c(("hpcg", 16), *S256, "mgpoly", steps=1, levels=None, ratio=4.0, galerkin="device"),
    "cd32_sell_64_256_poly_3_16": _c(("cd", 32, 32, 32), *S256, "poly", steps=3, ratio=16.0),
})
HOST_CASES = {name: c for name, c in CASES.items() if not c.get("device_product")}

# k to eps = 1e-10 ||b|| at itermax 300 (DESIGN 4.18's table; the issue's CPU sketch).  (matrix, format) -> column -> k; the
# columns: "none", "jacobi" (bicgstab_ref.solve), "sgs", ("poly", steps) at ratio 16, ("mgpoly", steps): scipy's P^T A P, omega = 1,
# the automatic depth, ratio 4
CRS = FORMATS["crs"]
TABLE = {
    (CD16, CRS): {"none": 46, "jacobi": 46, "sgs": 23, ("poly", 2): 25, ("poly", 3): 18, ("poly", 4): 14, ("mgpoly", 1): 13, ("mgpoly", 2): 9},
    (SCD16, CRS): {"none": 93, "jacobi": 46, "sgs": 23, ("poly", 2): 38, ("poly", 3): 28, ("poly", 4): 23, ("mgpoly", 1): 26,
                   ("mgpoly", 2): 17},
    (SCD16, S256): {"none": 97},
    (("cd", 32, 32, 32), CRS): {"none": 92, "jacobi": 92, "sgs": 47, ("poly", 2): 48, ("poly", 3): 32, ("poly", 4): 25, ("mgpoly", 1): 15,
                                ("mgpoly", 2): 28},
    (("hpcg", 16), CRS): {"none": 17, "jacobi": 17, "sgs": 13, ("poly", 2): 11, ("poly", 3): 10, ("poly", 4): 8, ("mgpoly", 1): 6,
                          ("mgpoly", 2): 5},
}


def table_case(matrix, f, column):
    """the case dict of a column of TABLE (itermax 300); "none" and "jacobi" are bicgstab_cases-style dicts"""
    if isinstance(column, str) and column != "sgs":
        return dict(matrix=matrix, fmt=f[0], C=f[1], sigma=f[2], precond=column, itermax=300, eps_rel=1e-10)
    if column == "sgs":
        return dict(_c(matrix, *f, "sgs"), itermax=300)
    kind, steps = column
    if kind == "poly":
        return dict(_c(matrix, *f, "poly", steps=steps, ratio=16.0), itermax=300)
    return dict(_c(matrix, *f, "mgpoly", steps=steps, levels=None, ratio=4.0, galerkin=True), itermax=300)
