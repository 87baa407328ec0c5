#!/usr/bin/env python3
"""The smoothed-aggregation hierarchy on one GPU: what its set-up costs and whether the V-cycle on it pays, against
Jacobi, the polynomial (3, 16) and -- on generated grids -- the trilinear device-Galerkin hierarchy IN THE SAME
PROCESS, by the method of DESIGN 4.12: fresh processes, same-process comparisons only, nothing gated.

    tools/aggregation_rate.py run [--cases hpcg:64:scs,hpcg:128:scs,irregular:80:crs] [--repeats 2] --out one_process.json
    tools/aggregation_rate.py merge p1.json p2.json p3.json --out profiles/aggregation_rate.json

`run` (one fresh process) reports per case
  - the set-up split per level: the aggregation's device ms (graph + rounds + joins), A T and the smoothing, the rest of
    sa_prolongation's wall time (the prefix sums, the counters' read-backs, the download of P), the Galerkin product's two stages
    and its host part, and the host convert + upload of Problem.from_csr; level sizes, rounds, strong entries, the longest row of P;
  - the rounds against a byte model as a fraction of 8 TB/s: a round is two launches, each gathers 4 B of column and 8 B of key per
    strong entry and reads and writes 8 B per row (+ 4 B of row pointer).  The rounds are gather- and latency-bound: the model says
    how far from a stream they are, it promises nothing.  The fraction divides the rounds' model by the WHOLE aggregation's device ms
    (graph, rounds -- each batch of four timed between its first and last launch, without the host's read-back -- and joins), so it
    is a lower bound on the rounds' own;
  - k and the loop ms to eps = 1e-10 ||b|| for Jacobi, the polynomial (3, 16), and at 1 and 2 steps the aggregation hierarchy and,
    on a generated grid, the trilinear device-Galerkin one, alternating, with the ratios to Jacobi of the same process.
An irregular case is first tried in a child process, because a row above the product's 1024-column capacity ends the process:
the refusal's message is recorded and the next smaller size tried (`--sizes`), and the first size that passes is measured.  Only
a refusal goes on to the next size -- status 1 with the library's `sbhip:` message last; any other end of the child ends the tool."""
import json
import os
import subprocess
import sys
import time

import ratelib
from ratelib import aggregation_levels, free, hostapi

NOTE = ("one entry per fresh process; only comparisons inside one process count (DESIGN 4.1).  Nothing is gated: the "
        "figures say what the aggregation hierarchy's set-up costs, where its time goes, and how the loop on it "
        "compares with Jacobi, the polynomial and the trilinear Galerkin hierarchy.  The byte model is a model")


def problem(kind, n, fmt):
    name = "generate" if kind == "hpcg" else "irregular"
    return hostapi.Problem(name, n, n, n, fmt=fmt, Cc=64, sigma=256 if fmt == "scs" else 1)


def probe(a):
    """child process: does the hierarchy of one case build?  prints its level sizes"""
    ratelib.capi.init(0)
    kind, n, fmt = a.case.split(":")
    p = problem(kind, int(n), fmt)
    coarse, rows = aggregation_levels(p)
    print(json.dumps([p.nr] + [q.nr for q, _, _ in coarse]))


def passing_size(a, kind, n, fmt):
    """the largest size of `--sizes` not above n whose hierarchy builds, and the refusals met on the way"""
    refusals = []
    for size in [n] + [s for s in a.sizes if s < n]:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "probe", "--case", "%s:%d:%s" % (kind, size, fmt)],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200)
        if out.returncode == 0:
            return size, refusals
        err = out.stderr.decode().strip().split("\n")
        if out.returncode != 1 or not err[-1].startswith("sbhip:"):  # an abort, a fault, a time limit: nothing more is started
            raise SystemExit("the probe of size %d ended with status %d and no refusal of the library's: %r" % (size, out.returncode, err[-3:]))
        refusals.append({"size": size, "status": out.returncode, "message": err[-1]})
        print("refused:", refusals[-1], file=sys.stderr, flush=True)
    raise SystemExit("no size of %r builds: %r" % (a.sizes, refusals))


def measure(a, kind, n, fmt):
    refusals = []
    if kind == "irregular":
        n, refusals = passing_size(a, kind, n, fmt)
    label = "%s%d %s" % (kind, n, "sell_64_256" if fmt == "scs" else "crs")
    p = problem(kind, n, fmt)
    secs, split, agg = [], None, None
    for _ in range(a.repeats):  # the last one is kept for the solves
        if agg:
            free(agg)
        t0 = time.perf_counter()
        agg, split = aggregation_levels(p)
        secs.append(round(time.perf_counter() - t0, 4))
    hier = {"aggregation": agg}
    tri_secs = None
    if kind == "hpcg":
        t0 = time.perf_counter()
        hier["trilinear_galerkin"] = hostapi.mg_galerkin(p, None, product="device")
        tri_secs = round(time.perf_counter() - t0, 4)
    eps = ratelib.rel_eps(p)
    solvers = {"jacobi": hostapi.PCG(p), "poly_3_16": hostapi.PCG(p, precond="poly", steps=3, ratio=16.0)}
    for w, coarse in hier.items():
        for steps in (1, 2):
            solvers["%s_s%d" % (w, steps)] = hostapi.PCG(p, precond="mgpoly", coarse=coarse, steps=steps)
    ks = ratelib.find_ks(solvers, a, eps)
    ms = ratelib.rounded(ratelib.to_eps_rounds(solvers, ks, eps, a.repeats + 1), 3)
    launches = {w: s.launches_per_body() for w, s in solvers.items()}
    for s in solvers.values():
        s.free()
    for coarse in hier.values():
        free(coarse)
    med = ratelib.medians(ms)
    out = {"problem": label, "rows": p.nr, "refusals": refusals, "level_rows": [p.nr] + [r["aggregates"] for r in split],
           "rounds": [r["rounds"] for r in split], "aggregation_setup_seconds": secs, "trilinear_galerkin_setup_seconds": tri_secs,
           "levels": split, "eps_rel": 1e-10, "k": ks, "launches_per_body": launches, "loop_ms_to_eps": ms, "loop_ms_to_eps_median": med,
           "loop_over_jacobi": {w: round(v / med["jacobi"], 4) for w, v in med.items()}}
    p.free()
    print("measured:", label, out["level_rows"], out["rounds"], ks, out["loop_over_jacobi"], file=sys.stderr, flush=True)
    return out


def run(a):
    L = ratelib.capi.init(0)
    out = dict(ratelib.process_header(L), cases=[])
    for item in a.cases.split(","):
        kind, n, fmt = item.split(":")
        out["cases"].append(measure(a, kind, int(n), fmt))
    ratelib.emit(out, a.out)


def merge(a):
    ratelib.merge_cases(a, NOTE)


def add_run_args(r):
    r.add_argument("--cases", default="hpcg:64:scs,hpcg:128:scs,irregular:80:crs")
    r.add_argument("--sizes", type=lambda s: [int(v) for v in s.split(",")], default=[64, 48, 40, 32, 24, 16, 12])


def main(parse=True):
    return ratelib.cli(run, merge, add_run_args, parse, also={"probe": (probe, lambda pr: pr.add_argument("--case", required=True))},
                       repeats=2, itermax=500, piece=5)


if __name__ == "__main__":
    main()
