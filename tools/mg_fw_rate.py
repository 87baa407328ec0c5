#!/usr/bin/env python3
"""PCG with the full-weighting V-cycle on one GPU against injection MG, SGS and Jacobi PCG IN THE SAME PROCESS.

    tools/mg_fw_rate.py run [--sizes 64 128 256] [--bodies 50] [--repeats 3] --out one_process.json
    tools/mg_fw_rate.py merge p1.json p2.json p3.json --out profiles/mg_fw_rate.json

tools/mg_rate.py's method with a fourth handle: `run` (one fresh process) creates a Jacobi, an SGS, an MG and an MG-fw handle per
problem -- HPCG n^3 in Sell-64-256 in the kernel mode the upload selects, the geometric hierarchy at auto depth, the trilinear P
and omega = 0.5 -- and reports
  - the levels, their rows and colours, and the set-up seconds of every handle;
  - launches per body, us per loop body (alternating windows of `bodies` bodies at eps = 0, timed on the device);
  - the apply (one V-cycle) alone: us, and TB/s of sb_pcg_precond_bytes (the byte model: a model, not a measurement);
  - k and the loop time to eps = 1e-10 ||b|| of every handle, and MG-fw's against the three others.
Nothing is gated: the tool says what the transfers cost and what they buy.  `merge` keeps every process's figures side by side;
only ratios taken inside one process count.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from sparsebench_amd import capi, hostapi, srchash  # noqa: E402
from sgs_rate import find_k, to_eps  # noqa: E402

NAMES = ("jacobi", "sgs", "mg", "mgfw")


def measure(a, label, p):
    solvers, setup = {}, {}
    for name in NAMES:
        t0 = time.perf_counter()
        solvers[name] = hostapi.PCG(p) if name == "jacobi" else hostapi.PCG(p, precond=name)
        setup[name] = round(time.perf_counter() - t0, 3)
        print("set up:", label, name, setup[name], "s", file=sys.stderr, flush=True)
    fw = solvers["mgfw"]
    bodies = a.bodies

    def timed(name):
        s = solvers[name]
        k = s.solve(bodies + 1, 0.0)
        ran = s.counters()["n_pAp"]
        if k != bodies + 1 or ran != bodies:
            raise RuntimeError("the timed loop did not run every body: %s k=%d bodies run %d" % (name, k, ran))
        return 1e3 * s.loop_ms() / bodies

    for name in NAMES:  # warm-up
        timed(name)
    us = {name: [] for name in NAMES}
    for _ in range(a.repeats):
        for name in NAMES:
            us[name].append(timed(name))
    med = {name: statistics.median(v) for name, v in us.items()}
    apply_us = {name: 1e3 * s.apply_ms(a.apply_reps) for name, s in solvers.items()}
    b = p.rhs()[0]
    eps = 1e-10 * float(np.linalg.norm(b))
    ks = {name: find_k(s, a.itermax, eps, a.piece) for name, s in solvers.items()}
    ms = {name: [] for name in NAMES}
    if all(1 < k < a.itermax for k in ks.values()):
        for _ in range(a.repeats):
            for name, s in solvers.items():
                ms[name].append(to_eps(s, ks[name], eps))
    mmed = {name: (statistics.median(v) if v else None) for name, v in ms.items()}
    ratio = lambda x, y: round(x / y, 4) if x and y else None  # noqa: E731
    nlev = fw.levels()
    out = {"problem": label, "rows": p.nr, "kernel_mode": p.pack_info()["mode"], "levels": nlev,
           "level_rows": [fw.level_rows(l) for l in range(nlev)], "level_colours": [fw.level_colours(l) for l in range(nlev)],
           "setup_seconds": setup,
           "launches_per_body": {name: s.launches_per_body() for name, s in solvers.items()},
           "bodies_per_window": bodies,
           "us_per_body": {name: [round(v, 2) for v in vals] for name, vals in us.items()},
           "us_per_body_median": {name: round(v, 2) for name, v in med.items()},
           "mgfw_over_body": {name: ratio(med["mgfw"], med[name]) for name in NAMES[:-1]},
           "precond_bytes": {name: int(s.precond_bytes()) for name, s in solvers.items()},
           "apply_us": {name: round(v, 2) for name, v in apply_us.items()},
           "apply_TBps_of_the_model": {name: round(s.precond_bytes() / (1e6 * apply_us[name]), 3) for name, s in solvers.items()},
           "mgfw_over_apply": {name: ratio(apply_us["mgfw"], apply_us[name]) for name in NAMES[:-1]},
           "eps_rel": 1e-10, "k": ks,
           "loop_ms_to_eps": {name: [round(v, 3) for v in vals] for name, vals in ms.items()},
           "loop_ms_to_eps_median": {name: (round(v, 3) if v is not None else None) for name, v in mmed.items()},
           "mgfw_over_time_to_eps": {name: ratio(mmed["mgfw"], mmed[name]) for name in NAMES[:-1]}}
    for s in solvers.values():
        s.free()
    print("measured:", label, json.dumps({k: out[k] for k in ("k", "us_per_body_median", "apply_us", "loop_ms_to_eps_median",
                                                               "mgfw_over_time_to_eps")}), file=sys.stderr, flush=True)
    return out


def run(a):
    L = capi.init(0)
    out = {"device": L.sb_device_name().decode(), "library": L.sb_version().decode(), "csrc_hash": srchash.csrc_hash(), "cases": []}
    for n in a.sizes:
        p = hostapi.Problem("generate", n, n, n, fmt="scs", Cc=64, sigma=256)
        out["cases"].append(measure(a, "hpcg%d" % n, p))
        p.free()
        if a.out:  # (kept after every size: a large one may be cut short)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


def merge(a):
    runs = [json.load(open(f)) for f in a.files]
    head = {k: runs[0][k] for k in ("library", "csrc_hash")}
    if any({k: r[k] for k in head} != head for r in runs):
        raise SystemExit("the runs do not describe the same build")
    out = dict(head, processes=len(runs), devices=sorted({r["device"] for r in runs}),
               note="one entry per fresh process; only ratios taken inside one process count (DESIGN 4.1).  Nothing is gated: "
                    "the figures say what a body with the full-weighting V-cycle costs against an injection MG, an SGS and a "
                    "Jacobi body and what it buys in iterations",
               runs=[r["cases"] for r in runs])
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256])
    r.add_argument("--bodies", type=int, default=50)
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
