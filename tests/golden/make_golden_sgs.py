#!/usr/bin/env python3
"""Writes tests/golden/sgs_hist.json from the CPU restatement of the SGS-PCG contract (tests/precond_ref.py) alone: per case of
tests/sgs_cases.py nC, k, the r.r / r.z / p.Ap histories as exact hex doubles and a SHA-256 of x; the iteration counts of Jacobi
and SGS PCG in the natural order; and the gap to scipy's preconditioned CG under the same operator.  Run from the repository
root:  python tests/golden/make_golden_sgs.py"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import pcg_ref  # noqa: E402
import precond_ref as ref  # noqa: E402
import sgs_cases  # noqa: E402
from test_sgs_host import scipy_gap  # noqa: E402

tmp = tempfile.mkdtemp(prefix="sgs_golden_")
out = {"_comment": "SGS-PCG histories of the CPU restatement (tests/precond_ref.py); made by tests/golden/make_golden_sgs.py",
       "cases": {}, "counts": {}, "scipy_gap": {}}
for name, c in sgs_cases.CASES.items():
    res = ref.run_case(ref.SGS, c, tmp)
    out["cases"][name] = pcg_ref.record(res)
    out["cases"][name]["nC"] = res["nC"]
    print(name, "k", res["k"], "nC", res["nC"], flush=True)
for name, c in sgs_cases.COUNT_CASES.items():
    plan, _, op, b, dinv, eps = ref.build_case(ref.SGS, c, tmp)
    out["counts"][name] = dict(k_jacobi=pcg_ref.solve(op, b, dinv, c["itermax"], eps)["k"],
                               k_sgs=ref.solve(op, plan, b, dinv, c["itermax"], eps)["k"], nC=plan.lev[0].smoother.nC)
    plan.free()
    print("counts", name, out["counts"][name], flush=True)
for name, c in sgs_cases.SCIPY_CASES.items():
    out["scipy_gap"][name] = scipy_gap(c, tmp)[0]
    print("scipy_gap", name, out["scipy_gap"][name], flush=True)
with open(os.path.join(HERE, "sgs_hist.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
