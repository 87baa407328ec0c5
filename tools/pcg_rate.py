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
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsebench_amd import capi, hostapi, srchash  # noqa: E402

PCG_EXTRA_BYTES_PER_ROW = 16.0  # r update: + dinv read, + z written
CG_VECTOR_BYTES_PER_ROW = 64.0  # 40 in the p update, 24 in the r update


def body_cost(L, a):
    n = a.n
    p = hostapi.Problem("generate", n, n, n, fmt="scs", Cc=64, sigma=256)
    solvers = {"cg_default": hostapi.CG(p, dot_order="tree"),
               "cg_five_launches": hostapi.CG(p, fuse_p=0, fuse_alpha=0, fuse_beta=0, dot_order="tree"),
               "pcg": hostapi.PCG(p)}
    bodies = a.bodies

    def timed(name):
        s = solvers[name]
        k = s.solve(bodies + 1, 0.0)
        ran = s.counters()["n_pAp"]
        if k != bodies + 1 or ran != bodies:
            raise RuntimeError("the timed loop did not run every body: %s k=%d bodies run %d" % (name, k, ran))
        return 1e3 * s.loop_ms() / bodies

    cg_model = L.sb_matrix_spmv_bytes(p.matrix) + CG_VECTOR_BYTES_PER_ROW * p.nr
    pcg_model = cg_model + PCG_EXTRA_BYTES_PER_ROW * p.nr
    out = {"problem": "hpcg%d" % n, "format": "Sell-64-256", "bodies_per_solve": bodies, "repeats": a.repeats,
           "model_bytes_per_body": {"cg": int(cg_model), "pcg": int(pcg_model)}, "model_ratio": round(pcg_model / cg_model, 4), "modes": {}}
    for mode in (5, 0):
        if p.use_packed(mode) != mode:
            raise RuntimeError("the matrix has no kernel mode %d" % mode)
        for name in solvers:  # warm-up
            timed(name)
        us = {name: [] for name in solvers}
        for _ in range(a.repeats):
            for name in solvers:
                us[name].append(timed(name))
        med = {name: statistics.median(v) for name, v in us.items()}
        out["modes"]["mode%d" % mode] = {
            "launches_per_body": {name: s.launches_per_body() for name, s in solvers.items()},
            "us_per_body": {name: [round(v, 2) for v in vals] for name, vals in us.items()},
            "us_per_body_median": {name: round(v, 2) for name, v in med.items()},
            "pcg_over_cg_five_launches": round(med["pcg"] / med["cg_five_launches"], 4),
            "pcg_over_cg_default": round(med["pcg"] / med["cg_default"], 4)}
    for s in solvers.values():
        s.free()
    p.free()
    return out


def find_k(s, itermax, eps, piece):
    """k at which the loop reaches eps (untimed; doubles as the warm-up solve): the solve in pieces, the stop flag read between
    them, so that a converged loop is not followed by thousands of no-op launches"""
    s.start(itermax, eps)
    done = 0
    while done < itermax - 1:
        s.run_iters(min(piece, itermax - 1 - done))
        done += piece
        if s.counters()["stop"]:
            break
    return s.finish()


def to_eps(s, k, eps):
    """loop_ms of the k - 1 bodies that reach eps: one blocking solve with itermax = k, which enqueues exactly those bodies and
    is timed on the device by the solver itself (no-op bodies and host polls would otherwise sit inside the interval)"""
    got = s.solve(k, eps)
    ran = s.counters()["n_pAp"]
    if got != k or ran != k - 1:
        raise RuntimeError("the timed solve did not run the %d bodies that reach eps: k=%d bodies run %d" % (k - 1, got, ran))
    return s.loop_ms()


def time_to_solution(L, a):
    nodes = a.nodes
    out = {"problem": "irregular, %d^3 nodes" % nodes, "eps_rel": 1e-10, "itermax": a.itermax, "piece": a.piece, "repeats": a.sol_repeats,
           "formats": {}}
    for label, fmt, sigma in (("crs", "crs", 1), ("sell_64_256", "scs", 256)):
        p = hostapi.Problem("irregular", nodes, nodes, nodes, fmt=fmt, Cc=64, sigma=sigma)
        eps = 1e-10 * math.sqrt(float(p.nr))  # b = 1 by the file rule: ||b|| = sqrt(nr)
        solvers = {"cg": hostapi.CG(p, dot_order="tree"), "pcg": hostapi.PCG(p)}
        ks = {name: find_k(s, a.itermax, eps, a.piece) for name, s in solvers.items()}
        for name, k in ks.items():
            if not 1 < k < a.itermax:
                raise RuntimeError("%s did not reach eps within itermax = %d on %s (k = %d)" % (name, a.itermax, label, k))
        ms = {n: [] for n in solvers}
        for _ in range(a.sol_repeats):
            for name, s in solvers.items():
                ms[name].append(to_eps(s, ks[name], eps))
        med = {n: statistics.median(v) for n, v in ms.items()}
        out["formats"][label] = {"rows": p.nr, "kernel_mode": p.pack_info()["mode"], "k_cg": ks["cg"], "k_pcg": ks["pcg"],
                                 "launches_per_body": {n: s.launches_per_body() for n, s in solvers.items()},
                                 "loop_ms": {n: [round(v, 3) for v in vals] for n, vals in ms.items()},
                                 "loop_ms_median": {n: round(v, 3) for n, v in med.items()},
                                 "pcg_over_cg_time_to_eps": round(med["pcg"] / med["cg"], 4),
                                 "pcg_over_cg_iterations": round(ks["pcg"] / ks["cg"], 4)}
        for s in solvers.values():
            s.free()
        p.free()
    return out


def run(a):
    L = capi.init(0)
    out = {"device": L.sb_device_name().decode(), "library": L.sb_version().decode(), "csrc_hash": srchash.csrc_hash()}
    if "a" in a.part:
        out["body_cost"] = body_cost(L, a)
    if "b" in a.part:
        out["time_to_solution"] = time_to_solution(L, a)
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
    if not all("body_cost" in r and "time_to_solution" in r for r in runs):
        raise SystemExit("every run must hold both measurements (run --part ab)")
    ratios = [f["pcg_over_cg_time_to_eps"] for r in runs for f in r["time_to_solution"]["formats"].values()]
    out = dict(head, processes=len(runs), devices=sorted({r["device"] for r in runs}),
               delivers=bool(len(runs) >= 3 and all(v < 1.0 for v in ratios)),
               note="one entry per fresh process; only ratios taken inside one process count (the CG loop itself moves by up to "
                    "1.24 x between processes with placement); delivers = the PCG loop time to eps is below the CG loop time to "
                    "eps in each of at least three processes, for both formats",
               body_cost=[r["body_cost"] for r in runs], time_to_solution=[r["time_to_solution"] for r in runs])
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--n", type=int, default=128)
    r.add_argument("--bodies", type=int, default=250)
    r.add_argument("--repeats", type=int, default=4)
    r.add_argument("--nodes", type=int, default=80)
    r.add_argument("--itermax", type=int, default=5000)
    r.add_argument("--piece", type=int, default=20)
    r.add_argument("--sol-repeats", dest="sol_repeats", type=int, default=3)
    r.add_argument("--part", default="ab")
    r.add_argument("--out", default=None)
    mg = sub.add_parser("merge")
    mg.add_argument("files", nargs="+")
    mg.add_argument("--out", required=True)
    a = ap.parse_args()
    (run if a.cmd == "run" else merge)(a)


if __name__ == "__main__":
    main()
