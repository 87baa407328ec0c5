"""Writes tests/golden/gmres_hist.json from the CPU restatement of the GMRES contract (tests/gmres_ref.py) alone:
per case k, both histories as exact doubles (hex) and a SHA-256 of x's bytes.  Two measured figures ride along, each asserted
by tests/test_gmres_host.py with a factor of 10: "scipy_gap" (max_k |res_ours[k] - res_scipy[k]| / ||b|| against
scipy.sparse.linalg.gmres) and "close_gap" (max over cycle closes of |sqrt(rr_true) - estimate| / ||b||).

    python tests/golden/make_golden_gmres.py            # every case (128^3 takes minutes)
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import gmres_cases  # noqa: E402
import gmres_ref  # noqa: E402


def main():
    tmp = tempfile.mkdtemp(prefix="gmres_golden_")
    out = {"cases": {}, "scipy_gap": {}, "close_gap": {}}
    for name in gmres_cases.CASES:
        r = gmres_ref.run_case(name, tmp)
        out["cases"][name] = gmres_ref.record(r)
        gaps = [abs(t - e) / r["bnorm"] for e, t in r["closes"]]
        out["close_gap"][name] = max(gaps) if gaps else 0.0
        if name in gmres_cases.SCIPY_CASES:
            out["scipy_gap"][name] = gmres_ref.scipy_gap(name, r, tmp)
        print(name, "k =", r["k"], "closes =", len(r["closes"]), "close_gap = %.3g" % out["close_gap"][name],
              "scipy_gap = %.3g" % out["scipy_gap"].get(name, float("nan")), flush=True)
    with open(os.path.join(HERE, "gmres_hist.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
