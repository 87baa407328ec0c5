#!/usr/bin/env python3
"""Writes tests/golden/precond_bytes.json: what the preconditioner handles of PCG report about themselves -- precond_bytes,
launches_per_body, levels, rows and colours per level -- for every case of tests/test_gpu_precond_bytes.py.  Unlike the other
goldens this one records the library, not a restatement: it pins the byte model as it stood when it was recorded (commit
2146f5f, before the three Sell-64 packers and their byte formulas were made one), so it is regenerated only when the model is
changed on purpose.  Needs a GPU: creating the handles is all it does.  Run from the repository root:
  python tests/golden/make_golden_precond_bytes.py [out.json]"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from sparsebench_amd import capi  # noqa: E402
from test_gpu_precond_bytes import cases, record  # noqa: E402

capi.init(0)
tmp = tempfile.mkdtemp(prefix="precond_bytes_golden_")
out = {"_comment": "sb_pcg_precond_bytes, sb_pcg_launches_per_body, levels, rows and colours of the PCG preconditioner handles as "
                   "the library reported them at commit 2146f5f; made by tests/golden/make_golden_precond_bytes.py",
       "cases": {}}
for key, matrix, f, handles in cases():
    out["cases"][key] = record(matrix, f[0], f[1], f[2], handles, tmp)
    print(key, {k: (v["bytes"], v["launches"]) for k, v in out["cases"][key].items()}, flush=True)
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "precond_bytes.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
