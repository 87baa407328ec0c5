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
import json
import sys
import time

import ratelib
from ratelib import hostapi, ratio

NAMES = ("jacobi", "sgs", "mg", "mgfw")
NOTE = ("one entry per fresh process; only ratios taken inside one process count (DESIGN 4.1).  Nothing is gated: "
        "the figures say what a body with the full-weighting V-cycle costs against an injection MG, an SGS and a "
        "Jacobi body and what it buys in iterations")


def measure(a, label, p):
    solvers, setup = {}, {}
    for name in NAMES:
        t0 = time.perf_counter()
        solvers[name] = hostapi.PCG(p) if name == "jacobi" else hostapi.PCG(p, precond=name)
        setup[name] = round(time.perf_counter() - t0, 3)
        print("set up:", label, name, setup[name], "s", file=sys.stderr, flush=True)
    fw = solvers["mgfw"]
    bodies = a.bodies
    us = ratelib.body_windows(solvers, NAMES, bodies, a.repeats)
    med = ratelib.medians(us)
    apply_us = {name: 1e3 * s.apply_ms(a.apply_reps) for name, s in solvers.items()}
    eps = ratelib.rel_eps(p)
    ks = ratelib.find_ks(solvers, a, eps)
    ms = ratelib.to_eps_rounds(solvers, ks, eps, a.repeats if all(ratelib.reached(ks, a.itermax).values()) else 0)
    mmed = ratelib.medians(ms)
    nlev = fw.levels()
    out = {"problem": label, "rows": p.nr, "kernel_mode": p.pack_info()["mode"], "levels": nlev,
           "level_rows": [fw.level_rows(l) for l in range(nlev)], "level_colours": [fw.level_colours(l) for l in range(nlev)],
           "setup_seconds": setup,
           "launches_per_body": {name: s.launches_per_body() for name, s in solvers.items()},
           "bodies_per_window": bodies,
           "us_per_body": ratelib.rounded(us, 2), "us_per_body_median": ratelib.rounded(med, 2),
           "mgfw_over_body": {name: ratio(med["mgfw"], med[name]) for name in NAMES[:-1]},
           "precond_bytes": {name: int(s.precond_bytes()) for name, s in solvers.items()},
           "apply_us": ratelib.rounded(apply_us, 2),
           "apply_TBps_of_the_model": {name: round(s.precond_bytes() / (1e6 * apply_us[name]), 3) for name, s in solvers.items()},
           "mgfw_over_apply": {name: ratio(apply_us["mgfw"], apply_us[name]) for name in NAMES[:-1]},
           "eps_rel": 1e-10, "k": ks,
           "loop_ms_to_eps": ratelib.rounded(ms, 3), "loop_ms_to_eps_median": ratelib.rounded(mmed, 3),
           "mgfw_over_time_to_eps": {name: ratio(mmed["mgfw"], mmed[name]) for name in NAMES[:-1]}}
    for s in solvers.values():
        s.free()
    print("measured:", label, json.dumps({k: out[k] for k in ("k", "us_per_body_median", "apply_us", "loop_ms_to_eps_median",
                                                               "mgfw_over_time_to_eps")}), file=sys.stderr, flush=True)
    return out


def run(a):
    L = ratelib.capi.init(0)
    out = dict(ratelib.process_header(L), cases=[])
    for n in a.sizes:
        p = hostapi.Problem("generate", n, n, n, **ratelib.FMT)
        out["cases"].append(measure(a, "hpcg%d" % n, p))
        p.free()
        ratelib.save(out, a.out)  # (kept after every size: a large one may be cut short)
    print(json.dumps(out))


def merge(a):
    ratelib.merge_cases(a, NOTE)


def main(parse=True):
    return ratelib.cli(run, merge, lambda r: r.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256]), parse,
                       bodies=50, repeats=3, apply_reps=20, itermax=5000, piece=10)


if __name__ == "__main__":
    main()
