#!/usr/bin/env python3
"""MG-preconditioned CG on one GPU against SGS and Jacobi PCG IN THE SAME PROCESS, on one problem.

    tools/mg_rate.py run [--n 128] [--small 64] [--bodies 100] [--repeats 3] --out one_process.json
    tools/mg_rate.py merge p1.json p2.json p3.json --out profiles/mg_rate.json

`run` (one fresh process) creates a Jacobi, an SGS and an MG handle (the geometric hierarchy at auto depth) per problem -- HPCG
n^3 in Sell-64-256 in both kernel modes (5: the masked row programs, 0: the reference-layout stream) and HPCG small^3 in the mode
the upload selects -- and reports for each, by tools/sgs_rate.py's method,
  - the levels, their rows and colours, and the set-up seconds of every handle (MG: the coarse matrices generated and uploaded,
    every level downloaded once, the host passes, the uploads of the sweep and restriction structures);
  - launches per body, us per loop body (alternating windows of `bodies` bodies at eps = 0, timed on the device) and the ratios;
  - the apply alone: us, and TB/s of sb_pcg_precond_bytes (the byte model: a model, not a measurement);
  - k and the loop time to eps = 1e-10 ||b|| of every handle, and MG's against both others.
Nothing is gated: the tool says what MG costs and what it buys.  `merge` keeps every process's figures side by side.
"""
import sys
import time

import ratelib
from ratelib import hostapi, ratio

NAMES = ("jacobi", "sgs", "mg")
NOTE = ("one entry per fresh process; only ratios taken inside one process count (DESIGN 4.1).  Nothing is gated: "
        "the figures say what an MG body costs against an SGS and a Jacobi body and what it buys in iterations")


def measure(L, a, label, p, mode):
    if mode is not None and p.use_packed(mode) != mode:
        raise RuntimeError("%s has no kernel mode %d" % (label, mode))
    solvers, setup = {}, {}
    for name in NAMES:
        t0 = time.perf_counter()
        solvers[name] = hostapi.PCG(p) if name == "jacobi" else hostapi.PCG(p, precond=name)
        setup[name] = round(time.perf_counter() - t0, 3)
    mg = solvers["mg"]
    bodies = a.bodies
    us = ratelib.body_windows(solvers, NAMES, bodies, a.repeats)
    med = ratelib.medians(us)
    apply_us = {name: 1e3 * s.apply_ms(a.apply_reps) for name, s in solvers.items()}
    eps = ratelib.rel_eps(p)
    ks = ratelib.find_ks(solvers, a, eps)
    ms = ratelib.to_eps_rounds(solvers, ks, eps, a.repeats if all(ratelib.reached(ks, a.itermax).values()) else 0)
    mmed = ratelib.medians(ms)
    nlev = mg.levels()
    out = {"problem": label, "rows": p.nr, "kernel_mode": p.pack_info()["mode"], "levels": nlev,
           "level_rows": [mg.level_rows(l) for l in range(nlev)], "level_colours": [mg.level_colours(l) for l in range(nlev)],
           "setup_seconds": setup,
           "launches_per_body": {name: s.launches_per_body() for name, s in solvers.items()},
           "bodies_per_window": bodies,
           "us_per_body": ratelib.rounded(us, 2), "us_per_body_median": ratelib.rounded(med, 2),
           "mg_over_jacobi_body": ratio(med["mg"], med["jacobi"]), "mg_over_sgs_body": ratio(med["mg"], med["sgs"]),
           "precond_bytes": {name: int(s.precond_bytes()) for name, s in solvers.items()},
           "apply_us": ratelib.rounded(apply_us, 2),
           "apply_TBps_of_the_model": {name: round(s.precond_bytes() / (1e6 * apply_us[name]), 3) for name, s in solvers.items()},
           "mg_over_sgs_apply": ratio(apply_us["mg"], apply_us["sgs"]),
           "eps_rel": 1e-10, "k": ks,
           "loop_ms_to_eps": ratelib.rounded(ms, 3), "loop_ms_to_eps_median": ratelib.rounded(mmed, 3),
           "mg_over_jacobi_time_to_eps": ratio(mmed["mg"], mmed["jacobi"]), "mg_over_sgs_time_to_eps": ratio(mmed["mg"], mmed["sgs"])}
    for s in solvers.values():
        s.free()
    print("measured:", label, file=sys.stderr, flush=True)
    return out


def run(a):
    L = ratelib.capi.init(0)
    out = dict(ratelib.process_header(L), cases=[])
    if a.n:
        p = hostapi.Problem("generate", a.n, a.n, a.n, **ratelib.FMT)
        for mode in (5, 0):
            out["cases"].append(measure(L, a, "hpcg%d mode %d" % (a.n, mode), p, mode))
        p.free()
    if a.small:
        p = hostapi.Problem("generate", a.small, a.small, a.small, **ratelib.FMT)
        out["cases"].append(measure(L, a, "hpcg%d" % a.small, p, None))
        p.free()
    ratelib.emit(out, a.out)


def merge(a):
    ratelib.merge_cases(a, NOTE)


def main(parse=True):
    return ratelib.cli(run, merge, None, parse, n=128, small=64, bodies=100, repeats=3, apply_reps=20, itermax=5000, piece=10)


if __name__ == "__main__":
    main()
