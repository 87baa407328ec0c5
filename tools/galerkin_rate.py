#!/usr/bin/env python3
"""The Galerkin hierarchy's set-up on one GPU, formed on the device against scipy and Matrix Market files IN THE
SAME PROCESS, by the method of DESIGN 4.12: fresh processes, same-process comparisons only, nothing gated.

    tools/galerkin_rate.py run [--cases 64:scs,128:scs,128:crs] [--repeats 2] --out one_process.json
    tools/galerkin_rate.py merge p1.json p2.json p3.json --out profiles/galerkin_rate.json

`run` (one fresh process) takes HPCG n^3 in Sell-64-256 or CRS per case at the deepest hierarchy and reports
  - the hierarchy's set-up seconds through scipy (hostapi.mg_galerkin: P^T A P, 17-digit files, Problem(file)) and through the
    device (product="device"), alternating, `repeats` times each;
  - the device path split per level: stage 1 and stage 2 device ms (sb_csr_stats), the rest of the product's wall time (the
    upload of P, the transpose of P on the host, the counts' prefix sums, the download and the zero-drop), and the host convert +
    upload of Problem.from_csr;
  - each stage against its byte model as a fraction of 8 TB/s.  The model is the compulsory traffic of the two launches of a stage
    with perfect reuse of the gathered rows: stage 1 reads A's stream (12 B per stored element) and P (12 B per entry, 8 B per
    row) in each launch and writes T once (12 B per entry, 8 B per row); stage 2 reads P^T and T in each launch and writes A_c.
    It is a model, not a measurement;
  - `level_kernel_modes` of both hierarchies: whether a coarse level made in memory gets row programs where a file level did not;
  - k and the loop ms to eps = 1e-10 ||b|| at 1 and 2 steps on both hierarchies.
The two hierarchies hold the same matrices, so their k must be identical: if one differs the tool exits with status 1."""
import shutil
import statistics
import sys
import tempfile
import time

import ratelib
from ratelib import free, hostapi

NOTE = ("one entry per fresh process; only comparisons inside one process count (DESIGN 4.1).  Nothing is gated: the "
        "figures say what the Galerkin hierarchy's set-up costs through scipy and files and through the device, and "
        "where the device path's time goes.  The byte models are models")


def measure(a, n, fmt):
    label = "hpcg%d %s" % (n, "sell_64_256" if fmt == "scs" else "crs")
    p = hostapi.Problem("generate", n, n, n, fmt=fmt, Cc=64, sigma=256 if fmt == "scs" else 1)
    nlev = hostapi.mg_levels(n, n, n)
    secs, split = {"scipy": [], "device": []}, None
    hier = {}
    for r in range(a.repeats):  # alternating; the last of each is kept for the solves
        for which in ("scipy", "device"):
            if which in hier:
                free(hier.pop(which)[0])
            tmp = tempfile.mkdtemp(prefix="galerkin_rate_") if which == "scipy" else None
            t0 = time.perf_counter()
            if which == "scipy":
                coarse = hostapi.mg_galerkin(p, nlev, tmp)
            else:
                coarse, split = ratelib.device_levels(p, nlev)
            secs[which].append(round(time.perf_counter() - t0, 4))
            hier[which] = (coarse, tmp)
    modes = {w: [q.pack_info()["mode"] for q in [p] + [c[0] for c in hier[w][0]]] for w in hier}
    progs = {w: [q.all_row_programs() for q in [p] + [c[0] for c in hier[w][0]]] for w in hier}
    eps = ratelib.rel_eps(p)
    ks, ms = {}, {}
    for steps in (1, 2):
        solvers = {"%s_s%d" % (w, steps): hostapi.PCG(p, precond="mgpoly", coarse=hier[w][0], steps=steps) for w in hier}
        ks.update(ratelib.find_ks(solvers, a, eps))
        ms.update(ratelib.rounded(ratelib.to_eps_rounds(solvers, ks, eps, a.repeats + 1), 3))
        for s in solvers.values():
            s.free()
    for w, (coarse, tmp) in hier.items():
        free(coarse)
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)
    out = {"problem": label, "rows": p.nr, "levels": nlev, "hierarchy_seconds": secs,
           "hierarchy_seconds_median": {w: statistics.median(v) for w, v in secs.items()},
           "device_over_scipy": round(statistics.median(secs["device"]) / statistics.median(secs["scipy"]), 4),
           "device_levels": split, "level_kernel_modes": modes, "level_all_row_programs": progs, "eps_rel": 1e-10, "k": ks,
           "loop_ms_to_eps": ms, "loop_ms_to_eps_median": ratelib.medians(ms)}
    p.free()
    print("measured:", label, out["hierarchy_seconds_median"], ks, file=sys.stderr, flush=True)
    return out


def run(a):
    L = ratelib.capi.init(0)
    out = dict(ratelib.process_header(L), cases=[])
    for item in a.cases.split(","):
        n, fmt = item.split(":")
        out["cases"].append(measure(a, int(n), fmt))
    ratelib.emit(out, a.out)
    bad = [(c["problem"], c["k"]) for c in out["cases"] for s in (1, 2) if c["k"]["scipy_s%d" % s] != c["k"]["device_s%d" % s]]
    if bad:
        print("k differs between the two hierarchies: %r" % (bad,), file=sys.stderr)
        sys.exit(1)


def merge(a):
    runs = ratelib.merge_cases(a, NOTE)
    ks = [c["k"] for r in runs for c in r["cases"]]
    if any(k["scipy_s%d" % s] != k["device_s%d" % s] for k in ks for s in (1, 2)):
        raise SystemExit("k differs between the two hierarchies")


def main(parse=True):
    return ratelib.cli(run, merge, lambda r: r.add_argument("--cases", default="64:scs,128:scs,128:crs"), parse,
                       repeats=2, itermax=500, piece=5)


if __name__ == "__main__":
    main()
