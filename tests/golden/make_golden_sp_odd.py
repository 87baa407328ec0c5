#!/usr/bin/env python3
"""Generate tests/golden/cg_hist_sp_ref_odd.json: every r.r / p.Ap of the reference's OWN single-precision solveCG (CRS) at two
HPCG shapes whose row counts are no multiple of 4: (33, 7, 5) -i 60 (1155 rows) and (19, 21, 23) -i 40 (9177 rows: more than
one 8192-element block of the seq dot).  Same recipe and format as cg_hist_sp_ref.json: oracle/build_ref_sp.sh
builds oracle/_ref/libsbref_crs_sp.so from the reference's sources where they lie (-DPRECISION=1, the strict flags, --wrap=ddot,
oracle/ref_shim.c); this script drives it through sbref_setup / sbref_solve_cg / sbref_hist_*.  The values are floats widened to
double, written with %.17e (exact).  With an argument: also re-derive those cases of cg_hist_sp_ref.json and compare (a check
of the recipe)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIB = os.path.join(ROOT, "oracle", "_ref", "libsbref_crs_sp.so")
OUT = os.path.join(ROOT, "tests", "golden", "cg_hist_sp_ref_odd.json")
CASES = [("hpcg33x7x5", (33, 7, 5), 60), ("hpcg19x21x23", (19, 21, 23), 40)]


def run(L, dims, itermax):
    L.sbref_setup(b"generate", dims[0], dims[1], dims[2], 1, 1)
    k = L.sbref_solve_cg(itermax, 0.0)
    rr, pap = [], []
    for i in range(L.sbref_hist_len()):
        (pap if L.sbref_hist_kind(i) else rr).append("%.17e" % L.sbref_hist_val(i))
    return {"itermax": itermax, "k": k, "rr": rr, "pAp": pap}


def main():
    L = C.CDLL(LIB)
    L.sbref_hist_val.restype = C.c_double
    L.sbref_solve_cg.argtypes = [C.c_int, C.c_double]
    for name in sys.argv[1:]:  # e.g. hpcg8 hpcg16: the recipe reproduces the committed cg_hist_sp_ref.json
        n = int(name[4:])
        g = json.load(open(os.path.join(ROOT, "tests", "golden", "cg_hist_sp_ref.json")))[name]
        got = run(L, (n, n, n), g["itermax"])
        vals = lambda c, a: repr([abs(float(v)) if v.lstrip("-") == "nan" else float(v) for v in c[a]])  # (NaN == NaN)
        same = got["k"] == g["k"] and all(vals(got, a) == vals(g, a) for a in ("rr", "pAp"))
        print("%s: %s" % (name, "reproduced" if same else "DIFFERS"))
        if not same:
            sys.exit(1)
    out = {}
    for name, dims, itermax in CASES:
        out[name] = run(L, dims, itermax)
        print("%s: k = %d, %d r.r, %d p.Ap" % (name, out[name]["k"], len(out[name]["rr"]), len(out[name]["pAp"])))
    json.dump(out, open(OUT, "w"), indent=0)


if __name__ == "__main__":
    main()
