#!/usr/bin/env python3
"""Writes tests/golden/poly_hist.json from the CPU restatement of the polynomial-PCG contract (tests/precond_ref.py) alone: per case
of tests/poly_cases.py the coefficients, k, the r.r / r.z / p.Ap histories as exact hex doubles and a SHA-256 of x; the iteration
counts of Jacobi and polynomial PCG in the natural order; and the gap to scipy's preconditioned CG under the same operator.  Run
from the repository root:  python tests/golden/make_golden_poly.py"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import pcg_ref  # noqa: E402
import poly_cases  # noqa: E402
import precond_ref as ref  # noqa: E402
from test_poly_host import scipy_gap  # noqa: E402

tmp = tempfile.mkdtemp(prefix="poly_golden_")
out = {"_comment": "polynomial-PCG histories of the CPU restatement (tests/precond_ref.py); made by tests/golden/make_golden_poly.py",
       "cases": {}, "counts": {}, "scipy_gap": {}}
for name, c in poly_cases.CASES.items():
    res = ref.run_case(ref.POLY, c, tmp)
    out["cases"][name] = pcg_ref.record(res)
    out["cases"][name]["coeffs"] = [float(v).hex() for v in res["coeffs"]]
    print(name, "k", res["k"], flush=True)
for name, c in poly_cases.COUNT_CASES.items():
    plan, _, op, b, dinv, eps = ref.build_case(ref.POLY, c, tmp)
    out["counts"][name] = dict(k_jacobi=pcg_ref.solve(op, b, dinv, c["itermax"], eps)["k"],
                               k_poly=ref.solve(op, plan, b, dinv, c["itermax"], eps)["k"])
    plan.free()
    print("counts", name, out["counts"][name], flush=True)
for name, c in poly_cases.SCIPY_CASES.items():
    out["scipy_gap"][name] = scipy_gap(c, tmp)[0]
    print("scipy_gap", name, out["scipy_gap"][name], flush=True)
with open(os.path.join(HERE, "poly_hist.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
