#!/usr/bin/env python3
"""Writes tests/golden/mg_hist.json from the CPU restatement of the MG-PCG contract (tests/precond_ref.py) alone: per case of
tests/mg_cases.py the levels, their rows and colour counts, k, the r.r / r.z / p.Ap histories as exact hex doubles and a SHA-256
of x; the iteration counts of Jacobi, SGS, the two sweeps without coarse levels and MG PCG; and the gap to scipy's preconditioned CG under the
same operator.  Run from the repository root:  python tests/golden/make_golden_mg.py"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import mg_cases  # noqa: E402
import precond_ref as ref  # noqa: E402
from test_mg_host import counts, golden_record, scipy_gap  # noqa: E402

tmp = tempfile.mkdtemp(prefix="mg_golden_")
out = {"_comment": "MG-PCG histories of the CPU restatement (tests/precond_ref.py); made by tests/golden/make_golden_mg.py",
       "cases": {}, "counts": {}, "scipy_gap": {}}
for name, c in mg_cases.CASES.items():
    res = ref.run_case(ref.MG, c, tmp)
    out["cases"][name] = golden_record(res)
    print(name, "k", res["k"], "L", res["L"], "nC", res["nC"], flush=True)
for name, c in mg_cases.COUNT_CASES.items():
    out["counts"][name] = counts(c, tmp)
    print("counts", name, out["counts"][name], flush=True)
for name in ("hpcg16_L4", "scaled16_over_hpcg8"):
    out["scipy_gap"][name] = scipy_gap(mg_cases.SCIPY_CASES[name], tmp)[0]
    print("scipy_gap", name, out["scipy_gap"][name], flush=True)
with open(os.path.join(HERE, "mg_hist.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
