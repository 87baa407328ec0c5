#!/usr/bin/env python3
"""Writes tests/golden/mg_poly_hist.json from the CPU restatement of the Chebyshev-smoothed V-cycle (tests/precond_ref.py) alone:
per case of tests/mg_poly_cases.py every level's coefficients, k, the r.r / r.z / p.Ap histories as exact hex doubles, a SHA-256 of
x, the launches per body and the byte model's count; the iteration counts of the Galerkin and the regenerated hierarchy at 16^3
and 32^3; DESIGN 4.16's count table at 16^3, 32^3 and 64^3; and the gap to scipy's preconditioned CG under the same operator.  Run from the repository root:
  python tests/golden/make_golden_mg_poly.py"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import mg_poly_cases as cases  # noqa: E402
from test_mg_poly_host import scipy_gap, golden_record, count  # noqa: E402
import precond_ref as ref  # noqa: E402

tmp = tempfile.mkdtemp(prefix="mg_poly_golden_")
out = {"_comment": "histories of PCG with the Chebyshev-smoothed V-cycle as the CPU restatement (tests/precond_ref.py) gives them; "
                   "made by tests/golden/make_golden_mg_poly.py", "cases": {}, "counts": {}, "scipy_gap": {}, "table": {}}
for name, c in cases.CASES.items():
    out["cases"][name] = golden_record(ref.run_case(ref.MGPOLY, c, tmp))
    print(name, "k", out["cases"][name]["k"], flush=True)
for name, c in cases.COUNT_CASES.items():
    out["counts"][name] = dict(zip(("k", "L"), count(c, tmp)))
    print("counts", name, out["counts"][name], flush=True)
for n in (16, 32, 64):
    out["table"][str(n)] = ref.count_table(n)
    print("table", n, out["table"][str(n)], flush=True)
for name, c in cases.SCIPY_CASES.items():
    out["scipy_gap"][name] = scipy_gap(c, tmp)[0]
    print("scipy_gap", name, out["scipy_gap"][name], flush=True)
with open(os.path.join(HERE, "mg_poly_hist.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
