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
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sparsebench_amd import capi, hostapi, srchash  # noqa: E402
from sgs_rate import find_k, to_eps  # noqa: E402

PEAK = 8.0e12  # B/s


def problem(kind, n, fmt):
    name = "generate" if kind == "hpcg" else "irregular"
    return hostapi.Problem(name, n, n, n, fmt=fmt, Cc=64, sigma=256 if fmt == "scs" else 1)


def aggregation_levels(p):
    """mg_aggregation spelled out, to time its parts per level"""
    fine, out, rows = p, [], []
    while len(out) + 1 < hostapi.MG_AGGREGATION_DEPTH and fine.nr > hostapi.MG_AGGREGATION_COARSEST:
        t0 = time.perf_counter()
        P, n_agg, st = hostapi.sa_prolongation(fine, stats=True)
        t1 = time.perf_counter()
        if 2 * n_agg > fine.nr:
            raise SystemExit("level %d: %d aggregates of %d rows: coarsens by less than 2" % (len(out), n_agg, fine.nr))
        (ptr, col, val), gst = hostapi.galerkin_product(fine, P, n_coarse=n_agg)
        t2 = time.perf_counter()
        q = hostapi.Problem.from_csr(ptr, col, val, fmt=p.fmt, Cc=p.Cc, sigma=p.sigma_arg)
        t3 = time.perf_counter()
        n, e = fine.nr, st["strong_entries"]
        model = st["rounds"] * 2 * (12.0 * e + 16.0 * n + 4.0 * (n + 1))
        dev = st["aggregate_ms"] + st["product_ms"] + st["smooth_ms"]
        rows.append({"level": len(out), "rows": n, "aggregates": n_agg, "rounds": st["rounds"], "strong_entries": e,
                     "nnz_p": len(P[1]), "max_row_p": st["max_row_p"], "max_row_at": gst["max_row_t"], "max_row_ac": gst["max_row_ac"],
                     "nnz_ac": len(col), "aggregate_ms": round(st["aggregate_ms"], 3), "product_ms": round(st["product_ms"], 3),
                     "smooth_ms": round(st["smooth_ms"], 3), "prolongation_host_ms": round(1e3 * (t1 - t0) - dev, 3),
                     "galerkin_stage_ms": round(gst["stage1_ms"] + gst["stage2_ms"], 3),
                     "galerkin_host_ms": round(1e3 * (t2 - t1) - gst["stage1_ms"] - gst["stage2_ms"], 3),
                     "convert_upload_ms": round(1e3 * (t3 - t2), 3), "rounds_model_bytes": int(model),
                     "aggregate_fraction_of_8TBps": round(model / (1e-3 * st["aggregate_ms"] * PEAK), 4)})
        out.append((q, P, 1.0))
        fine = q
    return out, rows


def free(coarse):
    for q, _, _ in coarse:
        q.free()


def probe(a):
    """child process: does the hierarchy of one case build?  prints its level sizes"""
    capi.init(0)
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
    b = p.rhs()[0]
    eps = 1e-10 * float(np.linalg.norm(b))
    solvers = {"jacobi": hostapi.PCG(p), "poly_3_16": hostapi.PCG(p, precond="poly", steps=3, ratio=16.0)}
    for w, coarse in hier.items():
        for steps in (1, 2):
            solvers["%s_s%d" % (w, steps)] = hostapi.PCG(p, precond="mgpoly", coarse=coarse, steps=steps)
    ks = {w: find_k(s, a.itermax, eps, a.piece) for w, s in solvers.items()}
    ms = {w: [] for w in solvers}
    for _ in range(a.repeats + 1):
        for w, s in solvers.items():
            ms[w].append(round(to_eps(s, ks[w], eps), 3))
    launches = {w: s.launches_per_body() for w, s in solvers.items()}
    for s in solvers.values():
        s.free()
    for coarse in hier.values():
        free(coarse)
    med = {w: statistics.median(v) for w, v in ms.items()}
    out = {"problem": label, "rows": p.nr, "refusals": refusals, "level_rows": [p.nr] + [r["aggregates"] for r in split],
           "rounds": [r["rounds"] for r in split], "aggregation_setup_seconds": secs, "trilinear_galerkin_setup_seconds": tri_secs,
           "levels": split, "eps_rel": 1e-10, "k": ks, "launches_per_body": launches, "loop_ms_to_eps": ms, "loop_ms_to_eps_median": med,
           "loop_over_jacobi": {w: round(v / med["jacobi"], 4) for w, v in med.items()}}
    p.free()
    print("measured:", label, out["level_rows"], out["rounds"], ks, out["loop_over_jacobi"], file=sys.stderr, flush=True)
    return out


def run(a):
    L = capi.init(0)
    out = {"device": L.sb_device_name().decode(), "library": L.sb_version().decode(), "csrc_hash": srchash.csrc_hash(), "cases": []}
    for item in a.cases.split(","):
        kind, n, fmt = item.split(":")
        out["cases"].append(measure(a, kind, int(n), fmt))
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
               note="one entry per fresh process; only comparisons inside one process count (DESIGN 4.1).  Nothing is gated: the "
                    "figures say what the aggregation hierarchy's set-up costs, where its time goes, and how the loop on it "
                    "compares with Jacobi, the polynomial and the trilinear Galerkin hierarchy.  The byte model is a model",
               runs=[r["cases"] for r in runs])
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--cases", default="hpcg:64:scs,hpcg:128:scs,irregular:80:crs")
    r.add_argument("--sizes", type=lambda s: [int(v) for v in s.split(",")], default=[64, 48, 40, 32, 24, 16, 12])
    r.add_argument("--repeats", type=int, default=2)
    r.add_argument("--itermax", type=int, default=500)
    r.add_argument("--piece", type=int, default=5)
    r.add_argument("--out", default=None)
    pr = sub.add_parser("probe")
    pr.add_argument("--case", required=True)
    mg = sub.add_parser("merge")
    mg.add_argument("files", nargs="+")
    mg.add_argument("--out", required=True)
    a = ap.parse_args()
    {"run": run, "probe": probe, "merge": merge}[a.cmd](a)


if __name__ == "__main__":
    main()
