#!/usr/bin/env python3
"""Writes tests/golden/galerkin_hist.json from the CPU restatement of the Galerkin product (tests/galerkin_ref.py) alone: per
hierarchy of galerkin_ref.GOLDEN_PRODUCTS and for the scaled 8^3 matrix, the cancelling and the underflowing case every A_c as
its nnz and a SHA-256 over the bytes of ptr / col / val, the entries dropped and the row maxima; and of the two-level solve on the
scaled matrix (precond_ref.Hierarchy over galerkin_ref's operator) at 1 and 2 steps, CRS order and Sell-64-256 order: k, the r.r /
r.z / p.Ap histories as exact hex doubles and a SHA-256 of x.  Run from the repository root:
  python tests/golden/make_golden_galerkin.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import galerkin_ref as gr  # noqa: E402
import pcg_ref  # noqa: E402
import precond_ref as mp  # noqa: E402


def products():
    out = {}
    for name, (dims, levels) in gr.GOLDEN_PRODUCTS.items():
        out[name] = [dict(gr.digest(Ac), dropped=d, maxima=list(m)) for Ac, d, m in gr.hierarchy(dims, levels)]
    from sparsebench_amd import hostapi
    for name, (A, P, nc) in (("scaled8", (gr.scaled_hpcg8(), hostapi.mg_trilinear(8, 8, 8), 64)), ("cancelling", gr.cancelling()),
                             ("underflowing", gr.underflowing())):
        Ac, d, m = gr.product(A, P, nc)
        out[name] = [dict(gr.digest(Ac), dropped=d, maxima=list(m))]
    return out


def solves():
    out = {}
    for fname, fmt in (("crs", ("crs", 64, 1)), ("sell_64_256", ("scs", 64, 256))):
        for steps in (1, 2):
            hier, op, b, eps = gr.scaled_case(fmt, steps)[:4]
            run = mp.solve(op, hier, b, op.to_orig(hier.dinv), 150, eps)
            run["eps"] = eps
            out["scaled8_%s_steps%d" % (fname, steps)] = pcg_ref.record(run)
            hier.free()
    return out


if __name__ == "__main__":
    rec = {"_comment": "Galerkin coarse operators and the two-level solve on them as the CPU restatement (tests/galerkin_ref.py, "
                       "tests/precond_ref.py) gives them; made by tests/golden/make_golden_galerkin.py",
           "products": products(), "solves": solves()}
    with open(os.path.join(HERE, "galerkin_hist.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print({k: v["k"] for k, v in rec["solves"].items()})
