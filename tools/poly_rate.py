#!/usr/bin/env python3
"""PCG with the Chebyshev polynomial preconditioner on one GPU against Jacobi and SGS PCG IN THE SAME PROCESS.

    tools/poly_rate.py run [--sizes 64,128] [--nodes 80] [--bodies 100] [--repeats 3] --out one_process.json
    tools/poly_rate.py merge p1.json p2.json p3.json --out profiles/poly_rate.json

`run` (one fresh process) takes HPCG n^3 in Sell-64-256 for every n of --sizes in both kernel modes (5: the masked row programs,
0: the reference-layout stream) and the irregular stand-in of nodes^3 nodes in Sell-64-256 in the mode the upload selects.  Per
problem it creates a Jacobi handle, an SGS handle and a polynomial handle for every steps in {2, 3, 4} and ratio in {4, 8, 16, 30}
and reports
  - us per loop body of Jacobi, SGS and the polynomial per steps (the body does not depend on ratio; taken at the default),
    alternating windows of `bodies` bodies at eps = 0, timed on the device between the end of the prologue and the last body, and
    their ratios to the Jacobi body;
  - the apply alone: us, and TB/s of sb_pcg_precond_bytes (the byte model: a model, not a measurement); beside it the matrix's
    own SpMV in the selected mode;
  - k and the loop ms to eps = 1e-10 ||b|| of every handle (the solve first runs in pieces to find k, then is timed with
    itermax = k: exactly the bodies that reach eps), and their ratios to Jacobi's.
Nothing is gated: the tool says what the polynomial costs and what it buys.  `merge` keeps every process's figures side by side.
"""
import sys
import time

import ratelib
from ratelib import hostapi

STEPS, RATIOS, DEFAULT_RATIO = (2, 3, 4), (4.0, 8.0, 16.0, 30.0), 16.0
NOTE = ("one entry per fresh process; only ratios taken inside one process count (DESIGN 4.1).  Nothing is gated: "
        "the figures say what a polynomial body costs against a Jacobi and an SGS body and what it buys in iterations")


def measure(L, a, label, p, mode):
    if mode is not None and p.use_packed(mode) != mode:
        raise RuntimeError("%s has no kernel mode %d" % (label, mode))
    t0 = time.perf_counter()
    solvers = {"jacobi": hostapi.PCG(p)}
    t1 = time.perf_counter()
    solvers["sgs"] = hostapi.PCG(p, precond="sgs")
    t2 = time.perf_counter()
    for steps in STEPS:
        for ratio in RATIOS:
            solvers["poly_s%d_r%g" % (steps, ratio)] = hostapi.PCG(p, precond="poly", steps=steps, ratio=ratio)
    t3 = time.perf_counter()
    body_names = ["jacobi", "sgs"] + ["poly_s%d_r%g" % (steps, DEFAULT_RATIO) for steps in STEPS]
    n, bodies = p.nr, a.bodies
    us = ratelib.body_windows(solvers, body_names, bodies, a.repeats)
    med = ratelib.medians(us)
    apply_us = {name: 1e3 * solvers[name].apply_ms(a.apply_reps) for name in body_names}
    mv_us = ratelib.spmv_us(L, p, a.apply_reps)
    eps = ratelib.rel_eps(p)
    ks = ratelib.find_ks(solvers, a, eps)
    ms = ratelib.to_eps_rounds(solvers, ks, eps, a.repeats, ratelib.reached(ks, a.itermax))
    mmed = ratelib.medians(ms)
    ratio_to = lambda d, name: ratelib.ratio(d[name], d["jacobi"])  # noqa: E731
    best = min((name for name in solvers if name.startswith("poly") and mmed[name]), key=lambda name: mmed[name], default=None)
    out = {"problem": label, "rows": n, "kernel_mode": p.pack_info()["mode"], "nC": solvers["sgs"].colours(),
           "lambda_max_bound": solvers["poly_s3_r16"].interval()[1],
           "setup_seconds": {"jacobi": round(t1 - t0, 3), "sgs": round(t2 - t1, 3), "poly_each": round((t3 - t2) / (len(STEPS) * len(RATIOS)), 4)},
           "launches_per_body": {name: solvers[name].launches_per_body() for name in body_names},
           "bodies_per_window": bodies,
           "us_per_body": ratelib.rounded(us, 2), "us_per_body_median": ratelib.rounded(med, 2),
           "body_over_jacobi": {name: ratio_to(med, name) for name in body_names},
           "precond_bytes": {name: int(solvers[name].precond_bytes()) for name in body_names},
           "apply_us": ratelib.rounded(apply_us, 2),
           "apply_TBps": {name: round(solvers[name].precond_bytes() / (1e6 * apply_us[name]), 3) for name in body_names},
           "spmv_us": round(mv_us, 2), "spmv_stream_bytes": int(p.stream_bytes()),
           "spmv_TBps": round(p.stream_bytes() / (1e6 * mv_us), 3),
           "eps_rel": 1e-10, "k": ks,
           "loop_ms_to_eps": ratelib.rounded(ms, 3), "loop_ms_to_eps_median": ratelib.rounded(mmed, 3),
           "time_to_eps_over_jacobi": {name: ratio_to(mmed, name) for name in solvers},
           "best_poly_to_eps": best}
    for s in solvers.values():
        s.free()
    print("measured:", label, file=sys.stderr, flush=True)
    return out


def run(a):
    L = ratelib.capi.init(0)
    out = dict(ratelib.process_header(L), cases=[])
    for n in [int(v) for v in a.sizes.split(",") if v]:
        p = hostapi.Problem("generate", n, n, n, **ratelib.FMT)
        for mode in (5, 0):
            out["cases"].append(measure(L, a, "hpcg%d mode %d" % (n, mode), p, mode))
        p.free()
    if a.nodes:
        p = hostapi.Problem("irregular", a.nodes, a.nodes, a.nodes, **ratelib.FMT)
        out["cases"].append(measure(L, a, "irregular, %d^3 nodes" % a.nodes, p, None))
        p.free()
    ratelib.emit(out, a.out)


def merge(a):
    ratelib.merge_cases(a, NOTE)


def main(parse=True):
    return ratelib.cli(run, merge, lambda r: r.add_argument("--sizes", default="64,128"), parse,
                       nodes=80, bodies=100, repeats=3, apply_reps=20, itermax=5000, piece=10)


if __name__ == "__main__":
    main()
