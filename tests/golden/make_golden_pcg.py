#!/usr/bin/env python3
"""Writes tests/golden/pcg_hist.json from the CPU restatement of the PCG contract (tests/pcg_ref.py) alone: per case of
tests/pcg_cases.py k, the r.r / r.z / p.Ap histories as exact hex doubles and a SHA-256 of x; and the gap to scipy's
preconditioned CG of the cases compared with it.  Run from the repository root:  python tests/golden/make_golden_pcg.py"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import pcg_cases  # noqa: E402
import pcg_ref  # noqa: E402
from test_pcg_host import scipy_gap  # noqa: E402

tmp = tempfile.mkdtemp(prefix="pcg_golden_")
out = {"_comment": "PCG histories of the CPU restatement (tests/pcg_ref.py); made by tests/golden/make_golden_pcg.py",
       "cases": {}, "scipy_gap": {}}
for name, c in pcg_cases.CASES.items():
    out["cases"][name] = pcg_ref.record(pcg_ref.run_case(c, tmp))
    print(name, "k", out["cases"][name]["k"], flush=True)
for name, c in pcg_cases.SCIPY_CASES.items():
    out["scipy_gap"][name] = scipy_gap(c, tmp)[0]
    print("scipy_gap", name, out["scipy_gap"][name], flush=True)
with open(os.path.join(HERE, "pcg_hist.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
