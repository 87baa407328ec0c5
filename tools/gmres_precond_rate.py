#!/usr/bin/env python3
"""Right-preconditioned GMRES(m) on one GPU against unpreconditioned GMRES(30) and Jacobi-BiCGStab IN THE SAME PROCESS.

    tools/gmres_precond_rate.py run --problem cd|hpcg [--cd 64] [--n 128] [--repeats 3] --out one_process.json
    tools/gmres_precond_rate.py merge p1.json ... --out profiles/gmres_precond_rate.json

`run` (one fresh process, ONE problem: upwind convection-diffusion `cd`^3 written to a temporary Matrix Market file, or the
generated HPCG stencil n^3; Sell-64-256, the kernel mode the upload selects) measures, for m in {10, 30} and each preconditioner
-- none, jacobi, sgs, poly (3 steps, ratio 16), mgpoly at 1 step on the regenerated hierarchy (generated problems only), on
device-formed Galerkin operators and on the aggregation hierarchy where it is accepted --
  k             to eps = 1e-10 ||b||: the solve in pieces with the stop flag read in between (doubles as the warm-up),
  loop_ms       of the timed solves, itermax = k: exactly the k - 1 steps that reach eps with their cycle closes, timed on the
                device between the end of the prologue and the last step (sb_gmres_loop_ms); the configurations alternate inside
                every repeat,
  us_per_step   loop_ms / (k - 1): the closes' share included,
  mid_step_launches  sb_gmres_launches_per_step at the middle cycle position,
  apply_ms      one application of the preconditioner alone (sb_pcg_apply_precond_ms, 10 back to back): once per step, once more
                per cycle close,
  over_gmres30  loop_ms over unpreconditioned GMRES(30)'s of the same process,
  over_bicgstab loop_ms over BiCGStab(precond="jacobi")'s of the same process; BiCGStab under the same plan runs beside each plan
                (`bicgstab_<plan>`).
No ratio is fixed in advance: `merge` records the range of every same-process ratio over the processes, losses included (between
processes a loop moves with placement, DESIGN 4.1: only same-process ratios count).
"""
import json
import os
import tempfile

import ratelib
from ratelib import FMT, hostapi

RESTARTS = (10, 30)
RATIOS = ("over_gmres30", "over_bicgstab", "us_per_step", "apply_ms")


def plans(p, generated, dims, owned, notes):
    """name -> PCG handle (None: no preconditioner); every solver borrows these"""
    M = {"none": None, "jacobi": hostapi.PCG(p), "sgs": hostapi.PCG(p, precond="sgs"),
         "poly_3_16": hostapi.PCG(p, precond="poly", steps=3, ratio=16.0)}
    if generated:
        M["mgpoly_1_regenerated"] = hostapi.PCG(p, precond="mgpoly", steps=1)
        M["mgpoly_1_galerkin"] = hostapi.PCG(p, precond="mgpoly", steps=1, galerkin="device")
    else:
        M["mgpoly_1_galerkin"] = hostapi.PCG(p, precond="mgpoly", steps=1, coarse=ratelib.galerkin_levels(p, dims, owned))
    try:
        M["mgpoly_1_aggregation"] = hostapi.PCG(p, precond="mgpoly", steps=1, coarsening="aggregation")
    except Exception as e:  # refused where a product's row outgrows its capacity: recorded, not hidden
        notes["mgpoly_1_aggregation"] = "refused: %s" % (str(e)[:200],)
    return M


def solvers_of(p, M):
    """name -> handle: GMRES(m) under every plan, BiCGStab under every plan"""
    s = {}
    for name, pcg in M.items():
        for m in RESTARTS:
            s["gmres%d_%s" % (m, name)] = hostapi.GMRES(p, restart=m) if pcg is None else hostapi.GMRES(p, restart=m, precond=pcg)
        if pcg is not None:
            s["bicgstab_%s" % name] = hostapi.BiCGStab(p, precond=pcg)
    return s


def measure(a, solvers, M, eps):
    ks = ratelib.find_ks(solvers, a, eps)
    reached = ratelib.reached(ks, a.itermax)
    for yard in ("gmres30_none", "bicgstab_jacobi"):
        if not reached[yard]:
            raise RuntimeError("the yardstick %s did not reach eps within itermax = %d (k = %d)" % (yard, a.itermax, ks[yard]))
    ms = ratelib.to_eps_rounds(solvers, ks, eps, a.repeats, reached, named=True)
    med = ratelib.medians(ms)
    out = {}
    for n, s in solvers.items():
        e = {"k": ks[n], "steps": ks[n] - 1, "reached_eps": reached[n]}
        plan = n.split("_", 1)[1]
        if ratelib.kind(s) == "gmres":
            m = s.restart()
            e.update(restart=m, mid_step_launches=s.launches_per_step(m // 2))
        else:
            e["launches_per_body"] = s.launches_per_body()
        if M.get(plan) is not None:
            e["apply_ms"] = round(M[plan].apply_ms(10), 4)
        if reached[n]:
            e.update(loop_ms=[round(v, 3) for v in ms[n]], loop_ms_median=round(med[n], 3),
                     us_per_step=round(1e3 * med[n] / (ks[n] - 1), 2), over_gmres30=round(med[n] / med["gmres30_none"], 4),
                     over_bicgstab=round(med[n] / med["bicgstab_jacobi"], 4))
        out[n] = e
    return out


def run(a):
    L = ratelib.capi.init(0)
    out = dict(ratelib.process_header(L), format="Sell-64-256", eps_rel=1e-10, repeats=a.repeats, notes={})
    owned = []
    if a.problem == "cd":
        with tempfile.TemporaryDirectory(prefix="gmres_precond_rate_") as d:
            p = hostapi.Problem(ratelib.write_convdiff(os.path.join(d, "cd_%d.mtx" % a.cd), a.cd), 1, 1, 1, **FMT)
        out["problem"], dims = "convection-diffusion %d^3" % a.cd, (a.cd,) * 3
    else:
        p = hostapi.Problem("generate", a.n, a.n, a.n, **FMT)
        out["problem"], dims = "hpcg%d" % a.n, (a.n,) * 3
    out["rows"], out["kernel_mode"] = p.nr, p.pack_info()["mode"]
    eps = ratelib.rel_eps(p)
    M = plans(p, a.problem == "hpcg", dims, owned, out["notes"])
    solvers = solvers_of(p, M)
    out["solvers"] = measure(a, solvers, M, eps)
    for s in solvers.values():
        s.free()
    for pcg in M.values():
        if pcg is not None:
            pcg.free()
    for q in owned:
        q.free()
    p.free()
    ratelib.emit(out, a.out)


def merge(a):
    runs = ratelib.load_runs(a.files)
    ranges = {}
    for r in runs:
        for name, e in r["solvers"].items():
            ratelib.collect(ranges.setdefault(r["problem"], {}), name, e, RATIOS)
    ratelib.ranges([slot for prob in ranges.values() for slot in prob.values()], RATIOS)
    note = ("one entry per fresh process and problem; over_gmres30 / over_bicgstab = loop time to eps = 1e-10 ||b|| over "
            "unpreconditioned GMRES(30)'s / BiCGStab(precond='jacobi')'s of the same process (below 1: it pays); ranges: "
            "[min, max] over the processes; no ratio was fixed in advance")
    ratelib.dump(dict(ratelib.merge_head(runs, note), ranges=ranges, runs=runs), a.out)
    print(json.dumps(ranges, indent=1))


def main(parse=True):
    return ratelib.cli(run, merge, lambda r: r.add_argument("--problem", choices=("cd", "hpcg"), required=True), parse,
                       n=128, cd=64, repeats=3, itermax=2000, piece=10)


if __name__ == "__main__":
    main()
