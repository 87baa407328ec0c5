#!/usr/bin/env python3
"""Writes tests/golden/aggregation_hist.json from the CPU restatement of the smoothed-aggregation prolongation
(tests/aggregation_ref.py) alone: per grid of aggregation_ref.GRIDS and per hand-made matrix n_agg, rounds, the rows left undecided
after every round and P as its nnz and a SHA-256 over the bytes of ptr / col / val; the table of iteration counts k to
eps = 1e-10 ||b|| (Jacobi, the polynomial (3, 16), the aggregation hierarchy at 1 and 2 steps, with the level sizes and rounds) on
HPCG 16^3 and 32^3 and the irregular stand-in at 12^3 under PCG and on the 16^3 convection-diffusion matrix under BiCGStab; and of
the solves the GPU tests repeat k, the histories as exact hex doubles and a SHA-256 of x.  Run from the repository root:
  python tests/golden/make_golden_aggregation.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import aggregation_cases as ac  # noqa: E402
import aggregation_ref as ar  # noqa: E402
import galerkin_ref as gr  # noqa: E402


def prolongations():
    out = {}
    for dims in ar.GRIDS:
        P, n_agg, rounds, info = ar.prolongation(gr.stencil(dims), info=True)
        out["dims_%d_%d_%d" % dims] = dict(ar.digest(P), n_agg=n_agg, rounds=rounds, left=info["left"])
    for name, make in ar.HAND_MADE.items():
        A, theta = make()
        P, n_agg, rounds, info = ar.prolongation(A, theta, lmax=ac.HAND_LMAX, info=True)
        out[name] = dict(ar.digest(P), n_agg=n_agg, rounds=rounds, left=info["left"])
    return out


if __name__ == "__main__":
    rec = {"_comment": "the smoothed-aggregation prolongation, its hierarchy and the solves on it as the CPU restatement "
                       "(tests/aggregation_ref.py, tests/precond_ref.py) gives them; made by tests/golden/make_golden_aggregation.py",
           "prolongations": prolongations(), "table": ac.table(), "solves": {name: ac.record(name) for name in ac.SOLVES}}
    with open(os.path.join(HERE, "aggregation_hist.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec["table"], indent=1))
    print({k: v["k"] for k, v in rec["solves"].items()})
