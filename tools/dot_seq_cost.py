"""Cost of the reference's dot order (dot_seq_k): microseconds per sequential dot, from the dot_pass phase of
sb_cg_phase_ms in seq solves (the reference's op list; two dots per loop body: r.r and p.Ap), at HPCG 32^3 and 128^3
(Sell-64-256) and on the irregular stand-in at 80^3 nodes (CRS).  One process, one GPU; prints one JSON line per case.
usage: python tools/dot_seq_cost.py [iterations]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsebench_amd import capi, hostapi  # noqa: E402


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    capi.init(0)
    for name, n, fmt, sigma in (("hpcg32", 32, "scs", 256), ("hpcg128", 128, "scs", 256), ("irregular80", 80, "crs", 1)):
        p = hostapi.Problem("irregular" if name.startswith("irregular") else "generate", n, n, n, fmt=fmt, Cc=64, sigma=sigma)
        cg = hostapi.CG(p, dot_order="seq")
        cg.solve(3, 0.0)  # (first launches, page-in)
        cg.phase_timing(True)
        cg.start(iters + 1)
        cg.run_iters(iters)
        cg.finish()
        ph = cg.phase_us()
        cg.phase_timing(False)
        us, count = ph["dot_pass"]
        print(json.dumps({"case": name, "fmt": fmt, "sigma": sigma, "rows": p.nr, "dots": count, "us_per_dot": round(us, 1),
                          "ns_per_element": round(1e3 * us / p.nr, 3), "spmv_us": round(ph["spmv"][0], 1)}), flush=True)
        cg.free(), p.free()


if __name__ == "__main__":
    main()
