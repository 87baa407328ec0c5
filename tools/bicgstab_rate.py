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
import argparse
import json
import math
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsebench_amd import capi, hostapi, srchash  # noqa: E402

VECTOR_STREAMS_PER_BODY = 23  # p update 6, rhat.v 2, s update 5, t.s / t.t 2, x / r update 8
CG_VECTOR_BYTES_PER_ROW = 64.0  # 40 in the p update, 24 in the r update
BODIES = {"bicgstab": "n_rv", "cg": "n_pAp", "gmres": "steps"}


def write_convdiff(path, n):
    """7-point upwind convection-diffusion on an n^3 grid: diagonal 6, the three lower neighbours -1.5, the three upper
    neighbours -0.5 (every value exact in binary), as a `general` Matrix Market file; b = 1 by the file rule"""
    idx = np.arange(n ** 3, dtype=np.int64)
    x, y, z = idx % n, (idx // n) % n, idx // (n * n)
    rows, cols, vals = [idx], [idx], [np.full(idx.shape, 6.0)]
    for coord, step in ((x, 1), (y, n), (z, n * n)):
        lo, hi = idx[coord > 0], idx[coord < n - 1]
        rows += [lo, hi]
        cols += [lo - step, hi + step]
        vals += [np.full(lo.shape, -1.5), np.full(hi.shape, -0.5)]
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((c, r))
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write("%d %d %d\n" % (n ** 3, n ** 3, len(r)))
        np.savetxt(f, np.column_stack((r[order] + 1, c[order] + 1, v[order])), fmt="%d %d %.1f")
    return path


def body_cost(L, a):
    n = a.n
    p = hostapi.Problem("generate", n, n, n, fmt="scs", Cc=64, sigma=256)
    solvers = {"cg": hostapi.CG(p, dot_order="tree"), "bicgstab": hostapi.BiCGStab(p)}
    bodies = a.bodies

    def timed(name):
        s = solvers[name]
        k = s.solve(bodies + 1, 0.0)
        ran = s.counters()[BODIES[name]]
        if k != bodies + 1 or ran != bodies:
            raise RuntimeError("the timed loop did not run every body: %s k=%d bodies run %d" % (name, k, ran))
        return 1e3 * s.loop_ms() / bodies

    spmv = L.sb_matrix_spmv_bytes(p.matrix)
    model = {"cg": spmv + CG_VECTOR_BYTES_PER_ROW * p.nr, "bicgstab": 2.0 * spmv + 8.0 * VECTOR_STREAMS_PER_BODY * p.nr}
    out = {"problem": "hpcg%d" % n, "format": "Sell-64-256", "bodies_per_solve": bodies, "repeats": a.repeats,
           "model_bytes_per_body": {k: int(v) for k, v in model.items()},
           "model_ratio_bicgstab_over_cg": round(model["bicgstab"] / model["cg"], 4), "modes": {}}
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
            "model_GBs_bicgstab": round(model["bicgstab"] / med["bicgstab"] / 1e3, 1),
            "bicgstab_over_cg": round(med["bicgstab"] / med["cg"], 4)}
    for s in solvers.values():
        s.free()
    p.free()
    return out


def find_k(name, s, itermax, eps, piece):
    """k at which the loop reaches eps (untimed; doubles as the warm-up solve): the solve in pieces, the stop flag read between
    them, so that a converged loop is not followed by thousands of no-op launches"""
    s.start(itermax, eps)
    done = 0
    while done < itermax - 1:
        cnt = min(piece, itermax - 1 - done)
        (s.run_steps if name == "gmres" else s.run_iters)(cnt)
        done += cnt
        if s.counters()["stop"]:
            break
    return s.finish()


def to_eps(name, s, k, eps):
    """loop_ms of the k - 1 bodies (steps) that reach eps: one blocking solve with itermax = k, timed on the device"""
    got = s.solve(k, eps)
    ran = s.counters()[BODIES[name]]
    if got != k or ran != k - 1:
        raise RuntimeError("the timed solve did not run the %d bodies that reach eps: %s k=%d bodies run %d" % (k - 1, name, got, ran))
    return s.loop_ms()


def time_to_eps(a, p, label, with_cg):
    b = p.rhs()[0]
    eps = 1e-10 * math.sqrt(float(np.dot(b, b)))
    solvers = {"bicgstab": hostapi.BiCGStab(p, precond="jacobi"), "gmres": hostapi.GMRES(p, restart=30)}
    if with_cg:
        solvers["cg"] = hostapi.CG(p, dot_order="tree")
    ks = {name: find_k(name, s, a.itermax, eps, a.piece) for name, s in solvers.items()}
    for name, k in ks.items():
        if not 1 < k < a.itermax:
            raise RuntimeError("%s did not reach eps within itermax = %d on %s (k = %d)" % (name, a.itermax, label, k))
    ms = {n: [] for n in solvers}
    for _ in range(a.sol_repeats):
        for name, s in solvers.items():
            ms[name].append(to_eps(name, s, ks[name], eps))
    med = {n: statistics.median(v) for n, v in ms.items()}
    out = {"problem": label, "format": "Sell-64-256", "rows": p.nr, "kernel_mode": p.pack_info()["mode"], "eps_rel": 1e-10,
           "k": ks, "spmvs": {n: (2 if n == "bicgstab" else 1) * (k - 1) for n, k in ks.items()},
           "loop_ms": {n: [round(v, 3) for v in vals] for n, vals in ms.items()},
           "loop_ms_median": {n: round(v, 3) for n, v in med.items()},
           "bicgstab_over_gmres_time_to_eps": round(med["bicgstab"] / med["gmres"], 4)}
    if with_cg:
        out["bicgstab_over_cg_time_to_eps"] = round(med["bicgstab"] / med["cg"], 4)
    for s in solvers.values():
        s.free()
    return out


def run(a):
    L = capi.init(0)
    out = {"device": L.sb_device_name().decode(), "library": L.sb_version().decode(), "csrc_hash": srchash.csrc_hash()}
    if "a" in a.part:
        out["body_cost"] = body_cost(L, a)
    if "b" in a.part:
        with tempfile.TemporaryDirectory(prefix="bicgstab_rate_") as d:
            path = write_convdiff(os.path.join(d, "cd_%d.mtx" % a.cd), a.cd)
            p = hostapi.Problem(path, 1, 1, 1, fmt="scs", Cc=64, sigma=256)
        out["convdiff"] = time_to_eps(a, p, "convection-diffusion %d^3" % a.cd, with_cg=False)
        p.free()
    if "c" in a.part:
        p = hostapi.Problem("generate", a.n, a.n, a.n, fmt="scs", Cc=64, sigma=256)
        out["hpcg"] = time_to_eps(a, p, "hpcg%d" % a.n, with_cg=True)
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
    if not all("body_cost" in r and "convdiff" in r and "hpcg" in r for r in runs):
        raise SystemExit("every run must hold the three measurements (run --part abc)")
    ratios = [r[m]["bicgstab_over_gmres_time_to_eps"] for r in runs for m in ("convdiff", "hpcg")]
    out = dict(head, processes=len(runs), devices=sorted({r["device"] for r in runs}),
               delivers=bool(len(runs) >= 3 and all(v < 1.0 for v in ratios)),
               note="one entry per fresh process; only ratios taken inside one process count (a loop moves by up to 1.24 x between "
                    "processes with placement); delivers = BiCGStab's loop time to eps is below GMRES(30)'s in each of at least "
                    "three processes, on convection-diffusion and on HPCG",
               body_cost=[r["body_cost"] for r in runs], convdiff=[r["convdiff"] for r in runs], hpcg=[r["hpcg"] for r in runs])
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--n", type=int, default=128)
    r.add_argument("--bodies", type=int, default=120)
    r.add_argument("--repeats", type=int, default=4)
    r.add_argument("--cd", type=int, default=64)
    r.add_argument("--itermax", type=int, default=2000)
    r.add_argument("--piece", type=int, default=10)
    r.add_argument("--sol-repeats", dest="sol_repeats", type=int, default=3)
    r.add_argument("--part", default="abc")
    r.add_argument("--out", default=None)
    mg = sub.add_parser("merge")
    mg.add_argument("files", nargs="+")
    mg.add_argument("--out", required=True)
    a = ap.parse_args()
    (run if a.cmd == "run" else merge)(a)


if __name__ == "__main__":
    main()
