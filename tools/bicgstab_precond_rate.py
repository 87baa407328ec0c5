#!/usr/bin/env python3
"""BiCGStab under PCG's preconditioner plans on one GPU against BiCGStab with the Jacobi diagonal IN THE SAME PROCESS.

    tools/bicgstab_precond_rate.py run --problem cd|hpcg [--cd 64] [--n 128] [--repeats 3] --out one_process.json
    tools/bicgstab_precond_rate.py merge p1.json ... --out profiles/bicgstab_precond_rate.json

`run` (one fresh process, ONE problem: upwind convection-diffusion `cd`^3 written to a temporary Matrix Market file, or the
generated HPCG stencil n^3; Sell-64-256) measures, in every kernel mode the matrix has (5: the masked row programs, 0: the
reference-layout stream), for each preconditioner -- none, Jacobi, sgs, poly (3 steps, ratio 16), poly (4, 30), mgpoly at 1 step on
the regenerated hierarchy (generated problems only) and on device-formed Galerkin operators --
  k            to eps = 1e-10 ||b||: the solve in pieces with the stop flag read in between (doubles as the warm-up),
  loop_ms      of the timed solves, itermax = k: exactly the k - 1 bodies that reach eps, timed on the device between the end of the
               prologue and the last body (sb_bicgstab_loop_ms); the preconditioners alternate inside every repeat,
  us_per_body  loop_ms / (k - 1),
  apply_ms     one application of the preconditioner alone (sb_pcg_apply_precond_ms, 10 back to back), twice per body,
  over_jacobi  loop_ms over BiCGStab(precond="jacobi")'s of the same process and mode: the yardstick.
On convection-diffusion GMRES(30) runs beside them.  No ratio is fixed in advance: `merge` records the range of every same-process
ratio over the processes (between processes a loop moves with placement, DESIGN 4.1: only same-process ratios count).
"""
import json
import os
import tempfile

import ratelib
from ratelib import FMT, hostapi

RATIOS = ("over_jacobi", "us_per_body", "apply_ms")


def handles(p, generated, dims, owned):
    """name -> BiCGStab handle (GMRES(30) beside them on the file matrix)"""
    h = {"none": hostapi.BiCGStab(p), "jacobi": hostapi.BiCGStab(p, precond="jacobi"), "sgs": hostapi.BiCGStab(p, precond="sgs"),
         "poly_3_16": hostapi.BiCGStab(p, precond="poly", steps=3, ratio=16.0),
         "poly_4_30": hostapi.BiCGStab(p, precond="poly", steps=4, ratio=30.0)}
    if generated:
        h["mgpoly_1_regenerated"] = hostapi.BiCGStab(p, precond="mgpoly", steps=1)
        h["mgpoly_1_galerkin"] = hostapi.BiCGStab(p, precond="mgpoly", steps=1, galerkin="device")
    else:
        h["mgpoly_1_galerkin"] = hostapi.BiCGStab(p, precond="mgpoly", steps=1, coarse=ratelib.galerkin_levels(p, dims, owned))
        h["gmres30"] = hostapi.GMRES(p, restart=30)
    return h


def measure(a, p, solvers, eps):
    ks = ratelib.find_ks(solvers, a, eps)
    reached = ratelib.reached(ks, a.itermax)
    ms = ratelib.to_eps_rounds(solvers, ks, eps, a.repeats, reached, named=True)
    med = ratelib.medians(ms)
    out = {}
    for n, s in solvers.items():
        e = {"k": ks[n], "reached_eps": reached[n]}
        if n != "gmres30":
            e["launches_per_body"] = s.launches_per_body()
            if getattr(s, "pcg", None) is not None:
                e["apply_ms"] = round(s.pcg.apply_ms(10), 4)
        if reached[n]:
            e.update(loop_ms=[round(v, 3) for v in ms[n]], loop_ms_median=round(med[n], 3),
                     us_per_body=round(1e3 * med[n] / (ks[n] - 1), 2), over_jacobi=round(med[n] / med["jacobi"], 4))
        out[n] = e
    return out


def run(a):
    L = ratelib.capi.init(0)
    out = dict(ratelib.process_header(L), format="Sell-64-256", eps_rel=1e-10, repeats=a.repeats)
    owned = []
    if a.problem == "cd":
        with tempfile.TemporaryDirectory(prefix="bicgstab_precond_rate_") as d:
            p = hostapi.Problem(ratelib.write_convdiff(os.path.join(d, "cd_%d.mtx" % a.cd), a.cd), 1, 1, 1, **FMT)
        out["problem"], dims = "convection-diffusion %d^3" % a.cd, (a.cd,) * 3
    else:
        p = hostapi.Problem("generate", a.n, a.n, a.n, **FMT)
        out["problem"], dims = "hpcg%d" % a.n, (a.n,) * 3
    out["rows"] = p.nr
    eps = ratelib.rel_eps(p)
    solvers = handles(p, a.problem == "hpcg", dims, owned)
    out["modes"] = {}
    for mode in sorted({p.use_packed(5), p.use_packed(0)}, reverse=True):
        if p.use_packed(mode) != mode:
            raise RuntimeError("the matrix has no kernel mode %d" % mode)
        out["modes"]["mode%d" % mode] = measure(a, p, solvers, eps)
    for s in solvers.values():
        s.free()
    for q in owned:
        q.free()
    p.free()
    ratelib.emit(out, a.out)


def merge(a):
    runs = ratelib.load_runs(a.files)
    ranges = {}
    for r in runs:
        for mode, rows in r["modes"].items():
            for name, e in rows.items():
                ratelib.collect(ranges.setdefault(r["problem"], {}).setdefault(mode, {}), name, e, RATIOS)
    ratelib.ranges([slot for prob in ranges.values() for rows in prob.values() for slot in rows.values()], RATIOS)
    note = ("one entry per fresh process and problem; over_jacobi = loop time to eps = 1e-10 ||b|| over "
            "BiCGStab(precond='jacobi') of the same process and kernel mode (below 1: the preconditioner pays); ranges: "
            "[min, max] over the processes; no ratio was fixed in advance")
    ratelib.dump(dict(ratelib.merge_head(runs, note), ranges=ranges, runs=runs), a.out)
    print(json.dumps(ranges, indent=1))


def main(parse=True):
    return ratelib.cli(run, merge, lambda r: r.add_argument("--problem", choices=("cd", "hpcg"), required=True), parse,
                       n=128, cd=64, repeats=3, itermax=2000, piece=10)


if __name__ == "__main__":
    main()
