#!/usr/bin/env python3
"""Generate tests/golden/ref_live.npz: what the reference build (oracle/_ref/libsbref_crs.so, oracle/build_ref.sh) computes in
the two cases tests/test_oracle_pinning.py pins the oracle on -- so that those tests also run where the reference was not built.

  gen_*  HPCG 12 x 10 x 9: fingerprint of its CRS arrays, SpMV / waxpby / ddot on vectors of np.random.default_rng(7), 40 CG
         iterations (k, r.r, p.Ap)
  irr12_csr_sha256  fingerprint of the CRS arrays the reference builds when it reads the irregular stand-in at 12^3 nodes
         exported as .mtx (its 40-iteration history is tests/golden/cg_hist_irregular_ref.json["irregular12"])

Needs oracle/_ref (the build container); a few seconds."""
import importlib.util
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pyoracle as po  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ref_live.npz")


def mk():
    spec = importlib.util.spec_from_file_location("mk", os.path.join(HERE, "make_golden_irregular_ref.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def vectors(nc, nr):
    rng = np.random.default_rng(7)
    return rng.standard_normal(nc), rng.standard_normal(nr)


def main():
    if not po.ref_available("crs"):
        sys.exit("oracle/_ref/libsbref_crs.so is not built here (oracle/build_ref.sh)")
    out, m = {}, mk()
    ref = po.Ref("crs")
    ref.setup("generate", 12, 10, 9)
    x, y = vectors(ref.nc, ref.nr)
    out["gen_csr_sha256"] = np.array(m.fingerprint(*ref.csr()))
    out["gen_spmv"] = ref.spmv(x)
    out["gen_waxpby"] = np.stack([ref.waxpby(1.0, y, -0.37, x), ref.waxpby(2.5, y, 1.0, x), ref.waxpby(2.5, y, -3.0, x)])
    out["gen_ddot"] = np.array(ref.ddot(x, y))
    h = ref.solve_cg(40)
    out["gen_cg_k"], out["gen_cg_rr"], out["gen_cg_pAp"] = np.array(h["k"]), h["rr"], h["pAp"]
    nr, nc, rp, col, val = m.stand_in(12)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "irregular_12.mtx")
        m.write_mtx(path, nr, rp, col, val)
        ref.setup(path)
        out["irr12_csr_sha256"] = np.array(m.fingerprint(*ref.csr()))
    np.savez(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
