"""Case list of the Chebyshev polynomial preconditioner's tests.  Matrices and formats are those of pcg_cases.CASES
(its "scale" case apart: the polynomial takes no caller's diagonal, so it would repeat hpcg16_sell_64_256); every small one is
solved twice, to eps = 1e-10 ||b|| and for 60 fixed iterations with eps = 0, at the default steps and ratio."""
import pcg_cases


def _c(matrix, fmt, C, sigma, itermax, eps_rel, **kw):
    return dict(matrix=matrix, fmt=fmt, C=C, sigma=sigma, itermax=itermax, eps_rel=eps_rel, **kw)


# the matrices and formats: name -> (matrix, fmt, C, sigma)
FORMATS = {n: (c["matrix"], c["fmt"], c["C"], c["sigma"]) for n, c in pcg_cases.CASES.items()
           if not c.get("big") and c["dinv"] == "jacobi"}

# the solves compared bit for bit on the GPU (tests/test_gpu_poly.py) and pinned in tests/golden/poly_hist.json
CASES = {}
for _n, _f in FORMATS.items():
    CASES[_n + "_eps"] = _c(*_f, 150, 1e-10)
    CASES[_n + "_60"] = _c(*_f, 60, 0.0)
CASES["hpcg128_sell_64_256_20"] = _c(("hpcg", 128), "scs", 64, 256, 20, 0.0, big=True)
SMALL = [n for n, c in CASES.items() if not c.get("big")]

# iteration counts to eps = 1e-10 ||b|| in the natural (CRS) order, Jacobi against the polynomial at steps = 3 (golden: "counts")
COUNT_CASES = {
    "hpcg16": _c(("hpcg", 16), "crs", 64, 1, 150, 1e-10),
    "scaled16": _c(("scaled", 16), "crs", 64, 1, 150, 1e-10),
}
SCIPY_CASES = {
    "irregular12": _c(("irregular", 12), "crs", 64, 1, 150, 1e-10),
    "scaled16": _c(("scaled", 16), "crs", 64, 1, 150, 1e-10),
    "hpcg16": _c(("hpcg", 16), "crs", 64, 1, 150, 1e-10),
}

# the bound and one apply (tests/test_gpu_poly_kernels.py): the matrices of pcg_cases.CASES in CRS, Sell-64-1, Sell-64-256 and
# Sell-4-8 (generic C)
APPLY_MATRICES = [("hpcg", 16), ("dims", 10, 11, 13), ("scaled", 8), ("scaled", 16), ("irregular", 12)]
APPLY_FORMATS = [("crs", 64, 1), ("scs", 64, 1), ("scs", 64, 256), ("scs", 4, 8)]
KERNEL_N = [1, 2, 127, 128, 255, 256, 257, 511, 513, 1000, 4097]
