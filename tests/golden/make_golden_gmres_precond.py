#!/usr/bin/env python3
"""Writes tests/golden/gmres_precond_hist.json from the CPU restatement of right-preconditioned GMRES(m)
(tests/gmres_precond_ref.py) alone: per host case of tests/gmres_precond_cases.py k, both histories as exact hex doubles, a
SHA-256 of x, eps and the launches at the first, a middle and the last cycle position; beside them the recorded gap to scipy's
GMRES on the same A M^-1 operator, the largest gap of a cycle close's estimate to its explicit residual (both relative to ||b||)
and the true residual over eps; and the iteration counts of DESIGN 4.20's table as the restatement gives them.  (The case whose
coarse matrix is the device's product of a file matrix has no entry: a GPU test restates it from the downloaded product.)  Run
from the repository root:  python tests/golden/make_golden_gmres_precond.py"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import gmres_precond_cases as cases  # noqa: E402
import gmres_precond_ref as ref  # noqa: E402

tmp = tempfile.mkdtemp(prefix="gmres_precond_golden_")
out = {"_comment": "GMRES(m) histories under PCG's preconditioners on the right, of the CPU restatement (tests/gmres_precond_ref.py); "
                   "made by tests/golden/make_golden_gmres_precond.py",
       "cases": {}, "table": {}}
for name, c in cases.HOST_CASES.items():
    run = ref.run_case(c, tmp)
    rec = ref.record(run)
    rec.update(scipy_gap=ref.scipy_gap(c, run, tmp), close_gap=ref.close_gap(run), true_residual_over_eps=ref.true_residual_ratio(run))
    out["cases"][name] = rec
    print(name, "k", rec["k"], "launches", rec["launches"], "scipy %.2e close %.2e true/eps %.3f"
          % (rec["scipy_gap"], rec["close_gap"], rec["true_residual_over_eps"]), flush=True)
for (matrix, m), row in cases.TABLE.items():
    for column in row:
        k = ref.run_case(cases.table_case(matrix, m, column), tmp)["k"]
        key = "%s m%d %s" % ("_".join(str(v) for v in matrix), m, column)
        out["table"][key] = int(k)
        print("table", key, k, flush=True)
with open(os.path.join(HERE, "gmres_precond_hist.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
