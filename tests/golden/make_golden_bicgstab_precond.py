#!/usr/bin/env python3
"""Writes tests/golden/bicgstab_precond_hist.json from the CPU restatement of BiCGStab under a preconditioner plan
(tests/bicgstab_precond_ref.py) alone: per host case of tests/bicgstab_precond_cases.py k, the five histories as exact hex doubles,
a SHA-256 of x, eps and the launches per body; and the iteration counts of DESIGN 4.18's table as the restatement gives them.  (The
case whose coarse matrix is the device's product of a file matrix has no entry: a GPU test restates it from the downloaded
product.)  Run from the repository root:  python tests/golden/make_golden_bicgstab_precond.py"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import bicgstab_precond_cases as cases  # noqa: E402
import bicgstab_precond_ref as ref  # noqa: E402
import bicgstab_ref  # noqa: E402

tmp = tempfile.mkdtemp(prefix="bicgstab_precond_golden_")
out = {"_comment": "BiCGStab histories under PCG's preconditioner plans, of the CPU restatement (tests/bicgstab_precond_ref.py); made "
                   "by tests/golden/make_golden_bicgstab_precond.py",
       "cases": {}, "table": {}}
for name, c in cases.HOST_CASES.items():
    out["cases"][name] = ref.record(ref.run_case(c, tmp))
    print(name, "k", out["cases"][name]["k"], "launches", out["cases"][name]["launches"], flush=True)
for (matrix, f), row in cases.TABLE.items():
    for column in row:
        c = cases.table_case(matrix, f, column)
        k = (bicgstab_ref.run_case(c, tmp) if column in ("none", "jacobi") else ref.run_case(c, tmp))["k"]
        key = "%s %s %s" % ("_".join(str(v) for v in matrix), "_".join(str(v) for v in f),
                            column if isinstance(column, str) else "%s_%d" % column)
        out["table"][key] = int(k)
        print("table", key, k, flush=True)
with open(os.path.join(HERE, "bicgstab_precond_hist.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
