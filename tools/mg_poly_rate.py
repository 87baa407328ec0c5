#!/usr/bin/env python3
"""PCG with the Chebyshev-smoothed V-cycle on one GPU against Jacobi, polynomial and MGFW PCG IN THE SAME PROCESS,
by the method of DESIGN 4.12 unchanged.

    tools/mg_poly_rate.py run [--sizes 64,128] [--bodies 100] [--repeats 3] --out one_process.json
    tools/mg_poly_rate.py merge p1.json p2.json p3.json --out profiles/mg_poly_rate.json

`run` (one fresh process) takes HPCG n^3 in Sell-64-256 for every n of --sizes in both kernel modes (5: the masked row programs,
0: the reference-layout stream; set on every level that has the mode).  Per problem it builds the regenerated hierarchy
(omega = 0.25) and the Galerkin one (hostapi.mg_galerkin) once and creates a Jacobi handle, a polynomial handle (3, 16), an MGFW
handle and an mgpoly handle for steps in {1, 2, 3} on each hierarchy, and reports
  - us per loop body of every handle: alternating windows of `bodies` bodies at eps = 0 after a warm-up, timed on the device
    between the end of the prologue and the last body, and their ratios to the Jacobi, the polynomial and the MGFW body (a
    handle whose r.r reaches exactly 0.0 before `bodies` bodies gets a shorter window: "bodies_per_window" says which);
  - k and the loop ms to eps = 1e-10 ||b|| (the solve first runs in pieces to find k, then is timed with itermax = k: exactly the
    bodies that reach eps), and the same three ratios;
  - the cycle alone: us per apply and TB/s of sb_pcg_precond_bytes (a model, not a measurement), and its split per level: the
    apply of the regenerated hierarchy cut off at 1, 2, .. L levels, whose differences are what each further level adds.
Nothing is gated: the tool says what the cycle costs and what it buys.  `merge` keeps every process's figures side by side.
"""
import shutil
import sys
import tempfile
import time

import ratelib
from ratelib import hostapi

STEPS = (1, 2, 3)
BASES = ("jacobi", "poly_s3_r16", "mgfw")
NOTE = ("one entry per fresh process; only ratios taken inside one process count (DESIGN 4.1).  Nothing is gated: the "
        "figures say what a body of the Chebyshev-smoothed cycle costs against a Jacobi, a polynomial and an MGFW body "
        "and what it buys in iterations")


def measure(L, a, label, p, mode, hier):
    level_modes = {}
    for name, coarse in hier.items():
        level_modes[name] = [q.use_packed(mode) for q in [p] + [c[0] for c in coarse]]
    if level_modes["regenerated"][0] != mode:
        raise RuntimeError("%s has no kernel mode %d" % (label, mode))
    for name, got in level_modes.items():  # a coarse level without the mode runs in the one it has: recorded, and said
        if any(m != mode for m in got):
            print("%s: the %s hierarchy's levels run in kernel modes %r" % (label, name, got), file=sys.stderr, flush=True)
    t = [time.perf_counter()]
    solvers = {"jacobi": hostapi.PCG(p)}
    t.append(time.perf_counter())
    solvers["poly_s3_r16"] = hostapi.PCG(p, precond="poly", steps=3, ratio=16.0)
    t.append(time.perf_counter())
    solvers["mgfw"] = hostapi.PCG(p, precond="mgfw", coarse=[(q, P, 0.5) for q, P, _ in hier["regenerated"]])
    t.append(time.perf_counter())
    for name, coarse in hier.items():
        for steps in STEPS:
            solvers["mgpoly_%s_s%d" % (name, steps)] = hostapi.PCG(p, precond="mgpoly", coarse=coarse, steps=steps)
    t.append(time.perf_counter())
    names, bodies = list(solvers), a.bodies

    # A cycle that converges by two decades per body drives the recurrence's r.r to exactly 0.0 before `bodies` bodies have run
    # (at eps = 0 the loop test normr > eps then ends the solve: 75 bodies at 64^3 with three steps on the Galerkin hierarchy).
    # Such a handle gets a shorter window, well inside what it runs: the warm-up finds it
    window = {}

    def timed(name):  # (ratelib.window_us with the window of its name)
        s = solvers[name]
        n_b = window.get(name, bodies)
        k = s.solve(n_b + 1, 0.0)
        ran = s.counters()["n_pAp"]
        if name not in window:  # the warm-up
            window[name] = bodies if ran == bodies else max(10, (ran - 10) // 10 * 10)
            return None
        if k != n_b + 1 or ran != n_b:
            raise RuntimeError("the timed loop did not run every body: %s k=%d bodies run %d of %d" % (name, k, ran, n_b))
        return 1e3 * s.loop_ms() / n_b

    def warm(name):  # twice where the window was shortened
        timed(name)
        if window[name] != bodies:
            timed(name)

    us = ratelib.alternate(names, a.repeats, timed, warm)
    med = ratelib.medians(us)
    apply_us = {name: 1e3 * solvers[name].apply_ms(a.apply_reps) for name in names}
    by_depth = {}
    for steps in STEPS:  # the cycle cut off at 1 .. L levels: the differences are what each further level adds
        row = []
        for depth in range(1, len(hier["regenerated"]) + 2):
            s = hostapi.PCG(p, precond="mgpoly", coarse=hier["regenerated"][:depth - 1], steps=steps)
            row.append(round(1e3 * s.apply_ms(a.apply_reps), 2))
            s.free()
        by_depth["s%d" % steps] = row
    mv_us = ratelib.spmv_us(L, p, a.apply_reps)
    eps = ratelib.rel_eps(p)
    ks = ratelib.find_ks(solvers, a, eps)
    ms = ratelib.to_eps_rounds(solvers, ks, eps, a.repeats, ratelib.reached(ks, a.itermax))
    mmed = ratelib.medians(ms)
    over = lambda d, base: {name: ratelib.ratio(d[name], d[base]) for name in names}  # noqa: E731
    out = {"problem": label, "rows": p.nr, "kernel_mode": p.pack_info()["mode"], "level_kernel_modes": level_modes,
           "level_rows": [p.nr] + [c[0].nr for c in hier["regenerated"]],
           "setup_seconds": {"jacobi": round(t[1] - t[0], 4), "poly": round(t[2] - t[1], 4), "mgfw": round(t[3] - t[2], 4),
                             "mgpoly_each": round((t[4] - t[3]) / (len(STEPS) * len(hier)), 4)},
           "launches_per_body": {name: solvers[name].launches_per_body() for name in names},
           "bodies_per_window": dict(window),
           "us_per_body": ratelib.rounded(us, 2), "us_per_body_median": ratelib.rounded(med, 2),
           "precond_bytes": {name: int(solvers[name].precond_bytes()) for name in names},
           "apply_us": ratelib.rounded(apply_us, 2),
           "apply_TBps": {name: round(solvers[name].precond_bytes() / (1e6 * apply_us[name]), 3) for name in names},
           "mgpoly_regenerated_apply_us_by_depth": by_depth,
           "spmv_us": round(mv_us, 2), "spmv_stream_bytes": int(p.stream_bytes()),
           "eps_rel": 1e-10, "k": ks,
           "loop_ms_to_eps": ratelib.rounded(ms, 3), "loop_ms_to_eps_median": ratelib.rounded(mmed, 3)}
    for base in BASES:
        out["body_over_" + base] = over(med, base)
        out["time_to_eps_over_" + base] = over(mmed, base)
    for s in solvers.values():
        s.free()
    print("measured:", label, file=sys.stderr, flush=True)
    return out


def run(a):
    L = ratelib.capi.init(0)
    out = dict(ratelib.process_header(L), cases=[])
    for n in [int(v) for v in a.sizes.split(",") if v]:
        p = hostapi.Problem("generate", n, n, n, **ratelib.FMT)
        nlev = hostapi.mg_levels(n, n, n)
        tmp = tempfile.mkdtemp(prefix="mg_poly_rate_")
        t0 = time.perf_counter()
        hier = {"regenerated": ratelib.regenerated(p, nlev)}
        t1 = time.perf_counter()
        hier["galerkin"] = hostapi.mg_galerkin(p, nlev, tmp)
        t2 = time.perf_counter()
        print("hierarchies of %d^3: regenerated %.2f s, galerkin %.2f s" % (n, t1 - t0, t2 - t1), file=sys.stderr, flush=True)
        for mode in (5, 0):
            case = measure(L, a, "hpcg%d mode %d" % (n, mode), p, mode, hier)
            case["hierarchy_seconds"] = {"regenerated": round(t1 - t0, 3), "galerkin_scipy_and_files": round(t2 - t1, 3)}
            out["cases"].append(case)
        for coarse in hier.values():
            ratelib.free(coarse)
        shutil.rmtree(tmp, ignore_errors=True)
        p.free()
    ratelib.emit(out, a.out)


def merge(a):
    ratelib.merge_cases(a, NOTE)


def main(parse=True):
    return ratelib.cli(run, merge, lambda r: r.add_argument("--sizes", default="64,128"), parse,
                       bodies=100, repeats=3, apply_reps=20, itermax=5000, piece=10)


if __name__ == "__main__":
    main()
