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
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sparsebench_amd import capi, hostapi, srchash  # noqa: E402
from sgs_rate import find_k, to_eps  # noqa: E402

PEAK = 8.0e12  # B/s


def stored(q):
    return q.nnzTrue if q.fmt == "crs" else q.nElems


def device_levels(p, nlev):
    """mg_galerkin(product="device") spelled out, to time its parts per level"""
    dims, fine, out, rows = p.dims, p, [], []
    for l in range(nlev - 1):
        P = hostapi.mg_trilinear(*dims)
        dims = tuple(d // 2 for d in dims)
        nc = dims[0] * dims[1] * dims[2]
        t0 = time.perf_counter()
        (ptr, col, val), st = hostapi.galerkin_product(fine, P, n_coarse=nc)
        t1 = time.perf_counter()
        q = hostapi.Problem.from_csr(ptr, col, val, fmt=p.fmt, Cc=p.Cc, sigma=p.sigma_arg)
        t2 = time.perf_counter()
        n, nnz_p, raw = fine.nr, len(P[1]), len(col) + st["dropped"]
        b1 = 2 * (12.0 * stored(fine) + 12.0 * nnz_p + 8.0 * n) + 12.0 * st["t_entries"] + 8.0 * n
        b2 = 2 * (12.0 * nnz_p + 8.0 * nc + 12.0 * st["t_entries"] + 8.0 * n) + 12.0 * raw + 8.0 * nc
        rows.append({"level": l + 1, "rows": nc, "nnz": len(col), "t_entries": st["t_entries"], "dropped": st["dropped"],
                     "max_row_t": st["max_row_t"], "max_row_ac": st["max_row_ac"],
                     "stage1_ms": round(st["stage1_ms"], 3), "stage2_ms": round(st["stage2_ms"], 3),
                     "product_host_ms": round(1e3 * (t1 - t0) - st["stage1_ms"] - st["stage2_ms"], 3),
                     "convert_upload_ms": round(1e3 * (t2 - t1), 3),
                     "stage1_model_bytes": int(b1), "stage2_model_bytes": int(b2),
                     "stage1_fraction_of_8TBps": round(b1 / (1e-3 * st["stage1_ms"] * PEAK), 4),
                     "stage2_fraction_of_8TBps": round(b2 / (1e-3 * st["stage2_ms"] * PEAK), 4)})
        out.append((q, P, 1.0))
        fine = q
    return out, rows


def free(coarse):
    for q, _, _ in coarse:
        q.free()


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
                coarse, split = device_levels(p, nlev)
            secs[which].append(round(time.perf_counter() - t0, 4))
            hier[which] = (coarse, tmp)
    modes = {w: [q.pack_info()["mode"] for q in [p] + [c[0] for c in hier[w][0]]] for w in hier}
    progs = {w: [q.all_row_programs() for q in [p] + [c[0] for c in hier[w][0]]] for w in hier}
    b = p.rhs()[0]
    eps = 1e-10 * float(np.linalg.norm(b))
    ks, ms = {}, {}
    for steps in (1, 2):
        solvers = {w: hostapi.PCG(p, precond="mgpoly", coarse=hier[w][0], steps=steps) for w in hier}
        for w, s in solvers.items():
            ks["%s_s%d" % (w, steps)] = find_k(s, a.itermax, eps, a.piece)
            ms["%s_s%d" % (w, steps)] = []
        for _ in range(a.repeats + 1):
            for w, s in solvers.items():
                ms["%s_s%d" % (w, steps)].append(round(to_eps(s, ks["%s_s%d" % (w, steps)], eps), 3))
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
           "loop_ms_to_eps": ms, "loop_ms_to_eps_median": {w: statistics.median(v) for w, v in ms.items()}}
    p.free()
    print("measured:", label, out["hierarchy_seconds_median"], ks, file=sys.stderr, flush=True)
    return out


def run(a):
    L = capi.init(0)
    out = {"device": L.sb_device_name().decode(), "library": L.sb_version().decode(), "csrc_hash": srchash.csrc_hash(), "cases": []}
    for item in a.cases.split(","):
        n, fmt = item.split(":")
        out["cases"].append(measure(a, int(n), fmt))
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    bad = [(c["problem"], c["k"]) for c in out["cases"] for s in (1, 2) if c["k"]["scipy_s%d" % s] != c["k"]["device_s%d" % s]]
    if bad:
        print("k differs between the two hierarchies: %r" % (bad,), file=sys.stderr)
        sys.exit(1)


def merge(a):
    runs = [json.load(open(f)) for f in a.files]
    head = {k: runs[0][k] for k in ("library", "csrc_hash")}
    if any({k: r[k] for k in head} != head for r in runs):
        raise SystemExit("the runs do not describe the same build")
    out = dict(head, processes=len(runs), devices=sorted({r["device"] for r in runs}),
               note="one entry per fresh process; only comparisons inside one process count (DESIGN 4.1).  Nothing is gated: the "
                    "figures say what the Galerkin hierarchy's set-up costs through scipy and files and through the device, and "
                    "where the device path's time goes.  The byte models are models",
               runs=[r["cases"] for r in runs])
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))
    ks = [c["k"] for r in runs for c in r["cases"]]
    if any(k["scipy_s%d" % s] != k["device_s%d" % s] for k in ks for s in (1, 2)):
        raise SystemExit("k differs between the two hierarchies")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--cases", default="64:scs,128:scs,128:crs")
    r.add_argument("--repeats", type=int, default=2)
    r.add_argument("--itermax", type=int, default=500)
    r.add_argument("--piece", type=int, default=5)
    r.add_argument("--out", default=None)
    mg = sub.add_parser("merge")
    mg.add_argument("files", nargs="+")
    mg.add_argument("--out", required=True)
    a = ap.parse_args()
    (run if a.cmd == "run" else merge)(a)


if __name__ == "__main__":
    main()
