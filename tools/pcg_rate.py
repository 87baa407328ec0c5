#!/usr/bin/env python3
"""Jacobi-preconditioned CG on one GPU against plain CG IN THE SAME PROCESS.

    tools/pcg_rate.py run [--n 128] [--bodies 250] [--repeats 4] [--nodes 80] [--part a|b|ab] --out one_process.json
    tools/pcg_rate.py merge p1.json p2.json p3.json --out profiles/pcg_rate.json

`run` (one fresh process) takes two measurements; in each the solvers alternate after a warm-up solve of each, and every
solve is timed on the device between the end of its prologue and its last body (sb_cg_loop_ms / sb_pcg_loop_ms).

(a) What a body costs: HPCG n^3, Sell-64-256, eps = 0, `repeats` x `bodies` loop bodies, in both kernel modes (5: the masked
    row programs, 0: the reference-layout stream).  PCG against hostapi.CG in the same mode twice: with fuse_alpha =
    fuse_beta = fuse_p = 0 (five launches with the scalar steps on their own, like for like) and with its defaults (what a
    user gets today).  Both ratios go beside the byte-model ratio: a PCG body moves 16 B/row more than a CG body (dinv read,
    z written, in the r update; the p update reads z where CG's reads r).  No pass mark: it says what a body costs.
(b) Time to solution: the irregular stand-in (`-m irregular`, nodes^3 nodes), CRS and Sell-64-256, b = 1, eps = 1e-10 ||b||.
    Each solver first runs to eps in pieces of `--piece` bodies with the stop flag read in between, which gives its k (and
    warms it up); the timed solves then run with itermax = k, exactly the k - 1 bodies that reach eps, so that no no-op
    launches behind the exit and no host polls sit inside the timed interval.  k_cg, k_pcg, loop_ms of each, their ratio.

`merge` keeps every process's figures side by side (between processes the CG loop itself moves by up to 1.24 x with
placement, DESIGN 4.1: only same-process ratios count) and writes `delivers`: the PCG loop time to eps is below the CG loop
time to eps in EVERY process, for both formats.
"""
import json

import ratelib
from ratelib import hostapi

PCG_EXTRA_BYTES_PER_ROW = 16.0  # r update: + dinv read, + z written
CG_VECTOR_BYTES_PER_ROW = 64.0  # 40 in the p update, 24 in the r update


def body_cost(L, a):
    n = a.n
    p = hostapi.Problem("generate", n, n, n, **ratelib.FMT)
    solvers = {"cg_default": hostapi.CG(p, dot_order="tree"),
               "cg_five_launches": hostapi.CG(p, fuse_p=0, fuse_alpha=0, fuse_beta=0, dot_order="tree"),
               "pcg": hostapi.PCG(p)}
    bodies = a.bodies
    cg_model = L.sb_matrix_spmv_bytes(p.matrix) + CG_VECTOR_BYTES_PER_ROW * p.nr
    pcg_model = cg_model + PCG_EXTRA_BYTES_PER_ROW * p.nr
    out = {"problem": "hpcg%d" % n, "format": "Sell-64-256", "bodies_per_solve": bodies, "repeats": a.repeats,
           "model_bytes_per_body": {"cg": int(cg_model), "pcg": int(pcg_model)}, "model_ratio": round(pcg_model / cg_model, 4), "modes": {}}
    for mode in (5, 0):
        if p.use_packed(mode) != mode:
            raise RuntimeError("the matrix has no kernel mode %d" % mode)
        us = ratelib.body_windows(solvers, list(solvers), bodies, a.repeats)
        med = ratelib.medians(us)
        out["modes"]["mode%d" % mode] = {
            "launches_per_body": {name: s.launches_per_body() for name, s in solvers.items()},
            "us_per_body": ratelib.rounded(us, 2), "us_per_body_median": ratelib.rounded(med, 2),
            "pcg_over_cg_five_launches": round(med["pcg"] / med["cg_five_launches"], 4),
            "pcg_over_cg_default": round(med["pcg"] / med["cg_default"], 4)}
    for s in solvers.values():
        s.free()
    p.free()
    return out


def time_to_solution(L, a):
    nodes = a.nodes
    out = {"problem": "irregular, %d^3 nodes" % nodes, "eps_rel": 1e-10, "itermax": a.itermax, "piece": a.piece, "repeats": a.sol_repeats,
           "formats": {}}
    for label, fmt, sigma in (("crs", "crs", 1), ("sell_64_256", "scs", 256)):
        p = hostapi.Problem("irregular", nodes, nodes, nodes, fmt=fmt, Cc=64, sigma=sigma)
        eps = ratelib.rel_eps(p)  # (b = 1 by the file rule: ||b|| = sqrt(nr))
        solvers = {"cg": hostapi.CG(p, dot_order="tree"), "pcg": hostapi.PCG(p)}
        ks = ratelib.find_ks(solvers, a, eps)
        for name, k in ks.items():
            if not 1 < k < a.itermax:
                raise RuntimeError("%s did not reach eps within itermax = %d on %s (k = %d)" % (name, a.itermax, label, k))
        ms = ratelib.to_eps_rounds(solvers, ks, eps, a.sol_repeats)
        med = ratelib.medians(ms)
        out["formats"][label] = {"rows": p.nr, "kernel_mode": p.pack_info()["mode"], "k_cg": ks["cg"], "k_pcg": ks["pcg"],
                                 "launches_per_body": {n: s.launches_per_body() for n, s in solvers.items()},
                                 "loop_ms": ratelib.rounded(ms, 3), "loop_ms_median": ratelib.rounded(med, 3),
                                 "pcg_over_cg_time_to_eps": round(med["pcg"] / med["cg"], 4),
                                 "pcg_over_cg_iterations": round(ks["pcg"] / ks["cg"], 4)}
        for s in solvers.values():
            s.free()
        p.free()
    return out


def run(a):
    L = ratelib.capi.init(0)
    out = ratelib.process_header(L)
    if "a" in a.part:
        out["body_cost"] = body_cost(L, a)
    if "b" in a.part:
        out["time_to_solution"] = time_to_solution(L, a)
    ratelib.emit(out, a.out)


def merge(a):
    runs = ratelib.load_runs(a.files)
    if not all("body_cost" in r and "time_to_solution" in r for r in runs):
        raise SystemExit("every run must hold both measurements (run --part ab)")
    ratios = [f["pcg_over_cg_time_to_eps"] for r in runs for f in r["time_to_solution"]["formats"].values()]
    note = ("one entry per fresh process; only ratios taken inside one process count (the CG loop itself moves by up to "
            "1.24 x between processes with placement); delivers = the PCG loop time to eps is below the CG loop time to "
            "eps in each of at least three processes, for both formats")
    out = dict(ratelib.merge_head(runs, note, delivers=bool(len(runs) >= 3 and all(v < 1.0 for v in ratios))),
               body_cost=[r["body_cost"] for r in runs], time_to_solution=[r["time_to_solution"] for r in runs])
    ratelib.dump(out, a.out)
    print(json.dumps(out))


def main(parse=True):
    return ratelib.cli(run, merge, lambda r: r.add_argument("--part", default="ab"), parse,
                       n=128, bodies=250, repeats=4, nodes=80, itermax=5000, piece=20, sol_repeats=3)


if __name__ == "__main__":
    main()
