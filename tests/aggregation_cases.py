"""Case list of the whole solves on the smoothed-aggregation hierarchy, shared by the CPU tests, the GPU tests and
tests/golden/make_golden_aggregation.py.  Every case runs to eps = 1e-10 ||b|| at itermax 150 with theta = 0, omega_s = 4/3, the
automatic depth and ratio 4; `steps` is the Chebyshev steps per smoothing.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import aggregation_ref as ar

ITERMAX = 150
HAND_LMAX = 2.0  # the hand-made matrices' lmax: the NaN matrix has no finite row-sum bound, and one value serves them all
CD16 = ("cd", 16, 16, 16)


def _c(solver, matrix, fname, steps):
    return dict(solver=solver, matrix=matrix, fmt=ar.FORMATS[fname], steps=steps)


SOLVES = {
    "pcg_hpcg16_crs_steps1": _c("pcg", ("hpcg", 16), "crs", 1),
    "pcg_hpcg16_sell_64_256_steps2": _c("pcg", ("hpcg", 16), "sell_64_256", 2),
    "pcg_irregular12_crs_steps1": _c("pcg", ("irregular", 12), "crs", 1),
    "pcg_irregular12_sell_64_256_steps2": _c("pcg", ("irregular", 12), "sell_64_256", 2),
    "pcg_scaled8_sell_64_256_steps2": _c("pcg", ("scaled8",), "sell_64_256", 2),
    "bicgstab_hpcg16_sell_64_256_steps1": _c("bicgstab", ("hpcg", 16), "sell_64_256", 1),
    "bicgstab_cd16_crs_steps2": _c("bicgstab", CD16, "crs", 2),
    "bicgstab_cd16_sell_64_256_steps1": _c("bicgstab", CD16, "sell_64_256", 1),
}


def gmatrix(matrix, tmpdir=None):
    """the oracle GMatrix of a case's matrix"""
    from oracle import pyoracle as po

    import bicgstab_ref as br
    import galerkin_ref as gr
    import pcg_ref
    if matrix[0] == "scaled8":
        ptr, col, val = gr.scaled_hpcg8()
        return po.GMatrix.from_csr(ptr.astype(np.uint32), col, val, nc=len(ptr) - 1)
    if matrix[0] == "cd":
        return br.gmatrix(matrix, tmpdir)
    return pcg_ref.gmatrix(matrix, tmpdir)


def problem(matrix, fmt, tmpdir=None):
    """the uploaded hostapi.Problem of a case's matrix"""
    import bicgstab_ref as br
    import galerkin_ref as gr
    import pcg_ref
    from sparsebench_amd import hostapi
    kw = dict(fmt=fmt[0], Cc=fmt[1], sigma=fmt[2])
    if matrix[0] == "scaled8":
        return hostapi.Problem.from_csr(*gr.scaled_hpcg8(), **kw)
    args = br.problem_args(matrix, tmpdir) if matrix[0] == "cd" else pcg_ref.problem_args(matrix, tmpdir)
    return hostapi.Problem(*args, **kw)


@functools.lru_cache(maxsize=None)
def levels_of(matrix):
    """(mats, steps) of aggregation_ref.hierarchy on a case's matrix: it does not depend on the format"""
    g = gmatrix(matrix)
    out = ar.hierarchy(ar.csr_of(g))
    g.free()
    return out


def run(c, itermax=ITERMAX):
    """the restatement's solve of a case: the dict of pcg_ref.solve / bicgstab_precond_ref.solve with eps, sizes, rounds"""
    import bicgstab_precond_ref as bpr
    import precond_ref as mp
    g = gmatrix(c["matrix"])
    hier, op, b, eps, (mats, st) = ar.build(g, c["fmt"], steps=c["steps"], found=levels_of(c["matrix"]))
    if c["solver"] == "pcg":
        out = mp.solve(op, hier, b, op.to_orig(hier.dinv), itermax, eps)
    else:
        out = bpr.solve(op, hier, b, itermax, eps)
        out["launches"] = bpr.launches_per_body(hier)
    out["eps"], out["rows"], out["rounds"] = eps, [len(M[0]) - 1 for M in mats], [s[2] for s in st]
    hier.free()
    return out


def record(name):
    import bicgstab_precond_ref as bpr
    import pcg_ref
    c = SOLVES[name]
    out = run(c)
    rec = pcg_ref.record(out) if c["solver"] == "pcg" else bpr.record(out)
    rec.update(rows=out["rows"], rounds=out["rounds"])
    return rec


TABLE_ROWS = {"hpcg16": ("pcg", ("hpcg", 16)), "hpcg32": ("pcg", ("hpcg", 32)), "irregular12": ("pcg", ("irregular", 12)),
              "cd16_bicgstab": ("bicgstab", CD16)}


def table_row(solver, matrix):
    """k at itermax 300 in CRS order: Jacobi, the polynomial (3, 16), the aggregation hierarchy at 1 and 2 steps; its level sizes
    and rounds"""
    import math

    from oracle import pyoracle as po

    import bicgstab_precond_ref as bpr
    import bicgstab_ref as br
    import pcg_ref
    import precond_ref as mp
    fmt = ar.FORMATS["crs"]
    g = gmatrix(matrix)
    op, b, dinv = pcg_ref.operator(g, *fmt), g.rhs(), pcg_ref.jacobi(g)
    eps = 1e-10 * math.sqrt(po.ddot_tree(op.to_dev(b), op.to_dev(b)))
    poly = mp.poly(g, op, 3, None, 16.0)
    if solver == "pcg":
        row = {"jacobi": int(pcg_ref.solve(op, b, dinv, 300, eps)["k"]), "poly_3_16": int(mp.solve(op, poly, b, dinv, 300, eps)["k"])}
    else:
        row = {"jacobi": int(br.solve(op, b, dinv, 300, eps)["k"]), "poly_3_16": int(bpr.solve(op, poly, b, 300, eps)["k"])}
    g.free()
    for steps in (1, 2):
        out = run(dict(solver=solver, matrix=matrix, fmt=fmt, steps=steps), 300)
        row["aggregation_steps%d" % steps] = int(out["k"])
        row["rows"], row["rounds"] = out["rows"], out["rounds"]
    return row


def table():
    return {name: table_row(*spec) for name, spec in TABLE_ROWS.items()}
