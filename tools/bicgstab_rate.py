#!/usr/bin/env python3
"""BiCGStab on one GPU against restarted GMRES(30) (and CG, where the matrix allows it) IN THE SAME PROCESS.

    tools/bicgstab_rate.py run [--n 128] [--bodies 120] [--repeats 4] [--cd 64] [--part a|b|c|abc] --out one_process.json
    tools/bicgstab_rate.py merge p1.json p2.json p3.json --out profiles/bicgstab_rate.json

`run` (one fresh process) takes three measurements; in each the solvers alternate after a warm-up solve of each, and every
solve is timed on the device between the end of its prologue and its last body (sb_*_loop_ms).

(a) What a body costs: HPCG n^3, Sell-64-256, eps = 0, `repeats` x `bodies` BiCGStab bodies (two SpMVs each) in both kernel
    modes (5: the masked row programs, 0: the reference-layout stream), beside hostapi.CG's body in the same mode and the byte
    model: 2 x sb_matrix_spmv_bytes (matrix, x read, y written) + 23 vector streams of 8 B/row.  No pass mark.
(b) Time to eps = 1e-10 ||b|| on upwind convection-diffusion `cd`^3 (non-symmetric, written to a temporary Matrix Market file,
    Sell-64-256), BiCGStab with the Jacobi preconditioner against hostapi.GMRES(restart=30).  Each solver first runs to eps in
    pieces with the stop flag read in between, which gives its k (and warms it up); the timed solves then run with itermax = k,
    exactly the bodies / Arnoldi steps that reach eps, so that no no-op launches and no host polls sit inside the interval.
(c) The same on HPCG n^3 (symmetric), with hostapi.CG as a third column.

`merge` keeps every process's figures side by side (between processes a loop moves by up to 1.24 x with placement, DESIGN
4.1: only same-process ratios count) and writes `delivers`: BiCGStab's loop time to eps is below GMRES(30)'s in EVERY one of
at least three processes, on both matrices.
"""
import json
import os
import tempfile

import ratelib
from ratelib import hostapi

VECTOR_STREAMS_PER_BODY = 23  # p update 6, rhat.v 2, s update 5, t.s / t.t 2, x / r update 8
CG_VECTOR_BYTES_PER_ROW = 64.0  # 40 in the p update, 24 in the r update


def body_cost(L, a):
    n = a.n
    p = hostapi.Problem("generate", n, n, n, **ratelib.FMT)
    solvers = {"cg": hostapi.CG(p, dot_order="tree"), "bicgstab": hostapi.BiCGStab(p)}
    bodies = a.bodies
    spmv = L.sb_matrix_spmv_bytes(p.matrix)
    model = {"cg": spmv + CG_VECTOR_BYTES_PER_ROW * p.nr, "bicgstab": 2.0 * spmv + 8.0 * VECTOR_STREAMS_PER_BODY * p.nr}
    out = {"problem": "hpcg%d" % n, "format": "Sell-64-256", "bodies_per_solve": bodies, "repeats": a.repeats,
           "model_bytes_per_body": {k: int(v) for k, v in model.items()},
           "model_ratio_bicgstab_over_cg": round(model["bicgstab"] / model["cg"], 4), "modes": {}}
    for mode in (5, 0):
        if p.use_packed(mode) != mode:
            raise RuntimeError("the matrix has no kernel mode %d" % mode)
        us = ratelib.body_windows(solvers, list(solvers), bodies, a.repeats)
        med = ratelib.medians(us)
        out["modes"]["mode%d" % mode] = {
            "launches_per_body": {name: s.launches_per_body() for name, s in solvers.items()},
            "us_per_body": ratelib.rounded(us, 2), "us_per_body_median": ratelib.rounded(med, 2),
            "model_GBs_bicgstab": round(model["bicgstab"] / med["bicgstab"] / 1e3, 1),
            "bicgstab_over_cg": round(med["bicgstab"] / med["cg"], 4)}
    for s in solvers.values():
        s.free()
    p.free()
    return out


def time_to_eps(a, p, label, with_cg):
    eps = ratelib.rel_eps(p)
    solvers = {"bicgstab": hostapi.BiCGStab(p, precond="jacobi"), "gmres": hostapi.GMRES(p, restart=30)}
    if with_cg:
        solvers["cg"] = hostapi.CG(p, dot_order="tree")
    ks = ratelib.find_ks(solvers, a, eps)
    for name, k in ks.items():
        if not 1 < k < a.itermax:
            raise RuntimeError("%s did not reach eps within itermax = %d on %s (k = %d)" % (name, a.itermax, label, k))
    ms = ratelib.to_eps_rounds(solvers, ks, eps, a.sol_repeats, named=True)
    med = ratelib.medians(ms)
    out = {"problem": label, "format": "Sell-64-256", "rows": p.nr, "kernel_mode": p.pack_info()["mode"], "eps_rel": 1e-10,
           "k": ks, "spmvs": {n: (2 if n == "bicgstab" else 1) * (k - 1) for n, k in ks.items()},
           "loop_ms": ratelib.rounded(ms, 3), "loop_ms_median": ratelib.rounded(med, 3),
           "bicgstab_over_gmres_time_to_eps": round(med["bicgstab"] / med["gmres"], 4)}
    if with_cg:
        out["bicgstab_over_cg_time_to_eps"] = round(med["bicgstab"] / med["cg"], 4)
    for s in solvers.values():
        s.free()
    return out


def run(a):
    L = ratelib.capi.init(0)
    out = ratelib.process_header(L)
    if "a" in a.part:
        out["body_cost"] = body_cost(L, a)
    if "b" in a.part:
        with tempfile.TemporaryDirectory(prefix="bicgstab_rate_") as d:
            path = ratelib.write_convdiff(os.path.join(d, "cd_%d.mtx" % a.cd), a.cd)
            p = hostapi.Problem(path, 1, 1, 1, **ratelib.FMT)
        out["convdiff"] = time_to_eps(a, p, "convection-diffusion %d^3" % a.cd, with_cg=False)
        p.free()
    if "c" in a.part:
        p = hostapi.Problem("generate", a.n, a.n, a.n, **ratelib.FMT)
        out["hpcg"] = time_to_eps(a, p, "hpcg%d" % a.n, with_cg=True)
        p.free()
    ratelib.emit(out, a.out)


def merge(a):
    runs = ratelib.load_runs(a.files)
    if not all("body_cost" in r and "convdiff" in r and "hpcg" in r for r in runs):
        raise SystemExit("every run must hold the three measurements (run --part abc)")
    ratios = [r[m]["bicgstab_over_gmres_time_to_eps"] for r in runs for m in ("convdiff", "hpcg")]
    note = ("one entry per fresh process; only ratios taken inside one process count (a loop moves by up to 1.24 x between "
            "processes with placement); delivers = BiCGStab's loop time to eps is below GMRES(30)'s in each of at least "
            "three processes, on convection-diffusion and on HPCG")
    out = dict(ratelib.merge_head(runs, note, delivers=bool(len(runs) >= 3 and all(v < 1.0 for v in ratios))),
               body_cost=[r["body_cost"] for r in runs], convdiff=[r["convdiff"] for r in runs], hpcg=[r["hpcg"] for r in runs])
    ratelib.dump(out, a.out)
    print(json.dumps(out))


def main(parse=True):
    return ratelib.cli(run, merge, lambda r: r.add_argument("--part", default="abc"), parse,
                       n=128, bodies=120, repeats=4, cd=64, itermax=2000, piece=10, sol_repeats=3)


if __name__ == "__main__":
    main()
