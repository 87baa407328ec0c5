#!/usr/bin/env python3
"""Writes tests/golden/mg_fw_hist.json from the CPU restatement of the V-cycle with full-weighting transfers (tests/precond_ref.py)
alone: per case of tests/mg_fw_cases.py the levels, their rows and colour counts, k, the r.r / r.z / p.Ap histories as exact hex
doubles and a SHA-256 of x; the iteration counts of Jacobi, SGS, the two sweeps and injection MG as tests/golden/mg_hist.json
holds them with this cycle's beside them; and the gap to scipy's preconditioned CG under the same operator.  Run from the
repository root:  python tests/golden/make_golden_mg_fw.py"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import mg_fw_cases  # noqa: E402
import precond_ref as ref  # noqa: E402
from test_mg_fw_host import count, golden_record, scipy_gap  # noqa: E402

tmp = tempfile.mkdtemp(prefix="mg_fw_golden_")
with open(os.path.join(HERE, "mg_hist.json")) as f:
    mg = json.load(f)
out = {"_comment": "MG-PCG histories with full-weighting transfers of the CPU restatement (tests/precond_ref.py); made by "
                   "tests/golden/make_golden_mg_fw.py",
       "cases": {}, "counts": {}, "scipy_gap": {}}
for name, c in mg_fw_cases.CASES.items():
    res = ref.run_case(ref.MGFW, c, tmp)
    out["cases"][name] = golden_record(res)
    print(name, "k", res["k"], "L", res["L"], "nC", res["nC"], flush=True)
for name, c in mg_fw_cases.COUNT_CASES.items():
    k, L = count(c, tmp)
    assert L == mg["counts"][name]["L"]
    out["counts"][name] = dict(mg["counts"][name], k_mgfw=k)
    print("counts", name, out["counts"][name], flush=True)
for name in ("hpcg16_L4", "scaled16_over_hpcg8"):
    out["scipy_gap"][name] = scipy_gap(mg_fw_cases.SCIPY_CASES[name], tmp)[0]
    print("scipy_gap", name, out["scipy_gap"][name], "injection's", mg["scipy_gap"][name], flush=True)
with open(os.path.join(HERE, "mg_fw_hist.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
