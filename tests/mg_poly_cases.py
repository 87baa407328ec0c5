"""Case list of the tests of the Chebyshev-smoothed V-cycle.  Matrices are named as pcg_cases names them; a case has
`levels` (the geometric hierarchy of a generated matrix at that depth with the trilinear P: regenerated stencils and
omega = 0.25, or with `galerkin` the operators P^T A P and omega = 1.0) or `coarse`: [(matrix, P, omega), ...] as mg_fw_cases has
it; `steps` and `coarse_steps` where they are not the defaults (2, and steps)."""
import mg_fw_cases
from mg_fw_cases import KERNEL_SHAPES, KERNEL_FORMATS, SELL_4_8_SHAPE, hand_made, hand_made_case, EMPTY_ROW, ZERO_WEIGHT_ROW  # noqa: F401
from poly_cases import KERNEL_N  # noqa: F401  (mgp_first_k stands on poly_step_k's skeleton: the same sizes)


def _c(matrix, fmt, C, sigma, itermax, eps_rel, **kw):
    return dict(matrix=matrix, fmt=fmt, C=C, sigma=sigma, itermax=itermax, eps_rel=eps_rel, **kw)


# the solves compared bit for bit on the GPU (tests/test_gpu_mg_poly.py) and pinned in tests/golden/mg_poly_hist.json: the twins
# of mg_fw_cases.CASES (the 32^3 case included), the other step counts on one of them, and the Galerkin hierarchy at 16^3
CASES = {n: dict(c) for n, c in mg_fw_cases.CASES.items()}
CASES["hpcg16_sell_64_256_L3_steps1"] = _c(("hpcg", 16), "scs", 64, 256, 150, 1e-10, levels=3, steps=1)
CASES["hpcg16_sell_64_256_L3_steps3_coarse1"] = _c(("hpcg", 16), "scs", 64, 256, 150, 1e-10, levels=3, steps=3, coarse_steps=1)
CASES["hpcg16_crs_L3_galerkin"] = _c(("hpcg", 16), "crs", 64, 1, 150, 1e-10, levels=3, galerkin=True)
CASES["hpcg16_sell_64_256_L3_galerkin"] = _c(("hpcg", 16), "scs", 64, 256, 150, 1e-10, levels=3, galerkin=True)
SMALL = [n for n, c in CASES.items() if not c.get("big")]

# one V-cycle and whole solves against an independent scipy formulation (golden: "scipy_gap"): mg_fw_cases.SCIPY_CASES' twins
SCIPY_CASES = {n: dict(c) for n, c in mg_fw_cases.SCIPY_CASES.items()}

# the claim the feature stands on (golden: "counts"): k to 1e-10 ||b|| at steps = 2, ratio = 4, the deepest hierarchy, natural order
COUNT_CASES = {
    "hpcg16_galerkin": _c(("hpcg", 16), "crs", 64, 1, 150, 1e-10, levels=None, galerkin=True),
    "hpcg32_galerkin": _c(("hpcg", 32), "crs", 64, 1, 150, 1e-10, levels=None, galerkin=True),
    "hpcg16_regenerated": _c(("hpcg", 16), "crs", 64, 1, 150, 1e-10, levels=None),
    "hpcg32_regenerated": _c(("hpcg", 32), "crs", 64, 1, 150, 1e-10, levels=None),
}
