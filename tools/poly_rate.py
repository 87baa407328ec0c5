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
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sparsebench_amd import capi, hostapi, srchash  # noqa: E402
from sgs_rate import find_k, spmv_us, to_eps  # noqa: E402

STEPS, RATIOS, DEFAULT_RATIO = (2, 3, 4), (4.0, 8.0, 16.0, 30.0), 16.0


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

    def timed(name):
        s = solvers[name]
        k = s.solve(bodies + 1, 0.0)
        ran = s.counters()["n_pAp"]
        if k != bodies + 1 or ran != bodies:
            raise RuntimeError("the timed loop did not run every body: %s k=%d bodies run %d" % (name, k, ran))
        return 1e3 * s.loop_ms() / bodies

    for name in body_names:  # warm-up
        timed(name)
    us = {name: [] for name in body_names}
    for _ in range(a.repeats):
        for name in body_names:
            us[name].append(timed(name))
    med = {name: statistics.median(v) for name, v in us.items()}
    apply_us = {name: 1e3 * solvers[name].apply_ms(a.apply_reps) for name in body_names}
    mv_us = spmv_us(L, p, a.apply_reps)
    b = p.rhs()[0]
    eps = 1e-10 * float(np.linalg.norm(b))
    ks = {name: find_k(s, a.itermax, eps, a.piece) for name, s in solvers.items()}
    ms = {name: [] for name in solvers}
    for _ in range(a.repeats):
        for name, s in solvers.items():
            if 1 < ks[name] < a.itermax:
                ms[name].append(to_eps(s, ks[name], eps))
    mmed = {name: (statistics.median(v) if v else None) for name, v in ms.items()}
    ratio_to = lambda d, name: round(d[name] / d["jacobi"], 4) if d[name] and d["jacobi"] else None  # noqa: E731
    best = min((name for name in solvers if name.startswith("poly") and mmed[name]), key=lambda name: mmed[name], default=None)
    out = {"problem": label, "rows": n, "kernel_mode": p.pack_info()["mode"], "nC": solvers["sgs"].colours(),
           "lambda_max_bound": solvers["poly_s3_r16"].interval()[1],
           "setup_seconds": {"jacobi": round(t1 - t0, 3), "sgs": round(t2 - t1, 3), "poly_each": round((t3 - t2) / (len(STEPS) * len(RATIOS)), 4)},
           "launches_per_body": {name: solvers[name].launches_per_body() for name in body_names},
           "bodies_per_window": bodies,
           "us_per_body": {name: [round(v, 2) for v in vals] for name, vals in us.items()},
           "us_per_body_median": {name: round(v, 2) for name, v in med.items()},
           "body_over_jacobi": {name: ratio_to(med, name) for name in body_names},
           "precond_bytes": {name: int(solvers[name].precond_bytes()) for name in body_names},
           "apply_us": {name: round(v, 2) for name, v in apply_us.items()},
           "apply_TBps": {name: round(solvers[name].precond_bytes() / (1e6 * apply_us[name]), 3) for name in body_names},
           "spmv_us": round(mv_us, 2), "spmv_stream_bytes": int(p.stream_bytes()),
           "spmv_TBps": round(p.stream_bytes() / (1e6 * mv_us), 3),
           "eps_rel": 1e-10, "k": ks,
           "loop_ms_to_eps": {name: [round(v, 3) for v in vals] for name, vals in ms.items()},
           "loop_ms_to_eps_median": {name: (round(v, 3) if v is not None else None) for name, v in mmed.items()},
           "time_to_eps_over_jacobi": {name: ratio_to(mmed, name) for name in solvers},
           "best_poly_to_eps": best}
    for s in solvers.values():
        s.free()
    print("measured:", label, file=sys.stderr, flush=True)
    return out


def run(a):
    L = capi.init(0)
    out = {"device": L.sb_device_name().decode(), "library": L.sb_version().decode(), "csrc_hash": srchash.csrc_hash(), "cases": []}
    for n in [int(v) for v in a.sizes.split(",") if v]:
        p = hostapi.Problem("generate", n, n, n, fmt="scs", Cc=64, sigma=256)
        for mode in (5, 0):
            out["cases"].append(measure(L, a, "hpcg%d mode %d" % (n, mode), p, mode))
        p.free()
    if a.nodes:
        p = hostapi.Problem("irregular", a.nodes, a.nodes, a.nodes, fmt="scs", Cc=64, sigma=256)
        out["cases"].append(measure(L, a, "irregular, %d^3 nodes" % a.nodes, p, None))
        p.free()
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


def merge(a):
    runs = [json.load(open(f)) for f in a.files]
    head = {k: runs[0][k] for k in ("library", "csrc_hash")}
    if any({k: r[k] for k in head} != head for r in runs):
        raise SystemExit("the runs do not describe the same build")
    out = dict(head, processes=len(runs), devices=sorted({r["device"] for r in runs}),
               note="one entry per fresh process; only ratios taken inside one process count (DESIGN 4.1).  Nothing is gated: "
                    "the figures say what a polynomial body costs against a Jacobi and an SGS body and what it buys in iterations",
               runs=[r["cases"] for r in runs])
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--sizes", default="64,128")
    r.add_argument("--nodes", type=int, default=80)
    r.add_argument("--bodies", type=int, default=100)
    r.add_argument("--repeats", type=int, default=3)
    r.add_argument("--apply-reps", dest="apply_reps", type=int, default=20)
    r.add_argument("--itermax", type=int, default=5000)
    r.add_argument("--piece", type=int, default=10)
    r.add_argument("--out", default=None)
    mg = sub.add_parser("merge")
    mg.add_argument("files", nargs="+")
    mg.add_argument("--out", required=True)
    a = ap.parse_args()
    (run if a.cmd == "run" else merge)(a)


if __name__ == "__main__":
    main()
