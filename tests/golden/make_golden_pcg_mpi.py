#!/usr/bin/env python3
"""Writes tests/golden/pcg_mpi_hist.json from the CPU restatement of PCG on P ranks (tests/pcg_mpi_ref.py) alone: per case of
pcg_mpi_ref.CASES k, the r.r / r.z / p.Ap histories as exact hex doubles, a SHA-256 of every rank's x and the polynomial's
interval; and the gap to scipy's preconditioned CG of the assembled systems compared with it.  Run from the repository root:
python tests/golden/make_golden_pcg_mpi.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import pcg_mpi_ref  # noqa: E402
from test_pcg_multirank_host import SCIPY_CASES, scipy_gap  # noqa: E402

out = {"_comment": "PCG histories of the P-rank CPU restatement (tests/pcg_mpi_ref.py); made by tests/golden/make_golden_pcg_mpi.py",
       "cases": {}, "scipy_gap": {}}
for name, c in pcg_mpi_ref.CASES.items():
    out["cases"][name] = pcg_mpi_ref.record(pcg_mpi_ref.run_case(c))
    print(name, "k", out["cases"][name]["k"], flush=True)
for name, c in SCIPY_CASES.items():
    out["scipy_gap"][name] = scipy_gap(c)[0]
    print("scipy_gap", name, out["scipy_gap"][name], flush=True)
with open(os.path.join(HERE, "pcg_mpi_hist.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
