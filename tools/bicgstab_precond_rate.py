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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sparsebench_amd import capi, hostapi, srchash  # noqa: E402
from bicgstab_rate import find_k, to_eps, write_convdiff  # noqa: E402

FMT = dict(fmt="scs", Cc=64, sigma=256)


def galerkin_levels(p, dims, owned):
    """[(Problem, P, 1.0), ...] of a FILE matrix on a known grid: the trilinear P and the device's P^T A P, to the depth the grid
    allows (a generated problem takes PCG(galerkin="device"))"""
    out, fine = [], p
    for _ in range(hostapi.mg_levels(*dims) - 1):
        P = hostapi.mg_trilinear(*dims)
        dims = tuple(d // 2 for d in dims)
        Ac, _ = hostapi.galerkin_product(fine, P, dims[0] * dims[1] * dims[2])
        q = hostapi.Problem.from_csr(*Ac, **FMT)
        owned.append(q)
        out.append((q, P, 1.0))
        fine = q
    return out


def handles(p, generated, dims, owned):
    """name -> BiCGStab handle (GMRES(30) beside them on the file matrix)"""
    h = {"none": hostapi.BiCGStab(p), "jacobi": hostapi.BiCGStab(p, precond="jacobi"), "sgs": hostapi.BiCGStab(p, precond="sgs"),
         "poly_3_16": hostapi.BiCGStab(p, precond="poly", steps=3, ratio=16.0),
         "poly_4_30": hostapi.BiCGStab(p, precond="poly", steps=4, ratio=30.0)}
    if generated:
        h["mgpoly_1_regenerated"] = hostapi.BiCGStab(p, precond="mgpoly", steps=1)
        h["mgpoly_1_galerkin"] = hostapi.BiCGStab(p, precond="mgpoly", steps=1, galerkin="device")
    else:
        h["mgpoly_1_galerkin"] = hostapi.BiCGStab(p, precond="mgpoly", steps=1, coarse=galerkin_levels(p, dims, owned))
        h["gmres30"] = hostapi.GMRES(p, restart=30)
    return h


def measure(a, p, solvers, eps):
    kind = lambda n: "gmres" if n == "gmres30" else "bicgstab"  # noqa: E731
    ks = {n: find_k(kind(n), s, a.itermax, eps, a.piece) for n, s in solvers.items()}
    reached = {n: 1 < k < a.itermax for n, k in ks.items()}
    ms = {n: [] for n in solvers if reached[n]}
    for _ in range(a.repeats):
        for n in ms:
            ms[n].append(to_eps(kind(n), solvers[n], ks[n], eps))
    med = {n: statistics.median(v) for n, v in ms.items()}
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
    L = capi.init(0)
    out = {"device": L.sb_device_name().decode(), "library": L.sb_version().decode(), "csrc_hash": srchash.csrc_hash(),
           "format": "Sell-64-256", "eps_rel": 1e-10, "repeats": a.repeats}
    owned = []
    if a.problem == "cd":
        with tempfile.TemporaryDirectory(prefix="bicgstab_precond_rate_") as d:
            p = hostapi.Problem(write_convdiff(os.path.join(d, "cd_%d.mtx" % a.cd), a.cd), 1, 1, 1, **FMT)
        out["problem"], dims = "convection-diffusion %d^3" % a.cd, (a.cd,) * 3
    else:
        p = hostapi.Problem("generate", a.n, a.n, a.n, **FMT)
        out["problem"], dims = "hpcg%d" % a.n, (a.n,) * 3
    out["rows"] = p.nr
    b = p.rhs()[0]
    eps = 1e-10 * math.sqrt(float(np.dot(b, b)))
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
    ranges = {}
    for r in runs:
        for mode, rows in r["modes"].items():
            for name, e in rows.items():
                slot = ranges.setdefault(r["problem"], {}).setdefault(mode, {}).setdefault(name, {"k": e["k"], "over_jacobi": [],
                                                                                                 "us_per_body": [], "apply_ms": []})
                if e["k"] != slot["k"]:
                    raise SystemExit("k of %s differs between processes" % name)
                for key in ("over_jacobi", "us_per_body", "apply_ms"):
                    if key in e:
                        slot[key].append(e[key])
    for prob in ranges.values():
        for rows in prob.values():
            for slot in rows.values():
                for key in ("over_jacobi", "us_per_body", "apply_ms"):
                    slot[key] = [min(slot[key]), max(slot[key])] if slot[key] else None
    out = dict(head, processes=len(runs), devices=sorted({r["device"] for r in runs}),
               note="one entry per fresh process and problem; over_jacobi = loop time to eps = 1e-10 ||b|| over "
                    "BiCGStab(precond='jacobi') of the same process and kernel mode (below 1: the preconditioner pays); ranges: "
                    "[min, max] over the processes; no ratio was fixed in advance",
               ranges=ranges, runs=runs)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(ranges, indent=1))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--problem", choices=("cd", "hpcg"), required=True)
    r.add_argument("--n", type=int, default=128)
    r.add_argument("--cd", type=int, default=64)
    r.add_argument("--repeats", type=int, default=3)
    r.add_argument("--itermax", type=int, default=2000)
    r.add_argument("--piece", type=int, default=10)
    r.add_argument("--out", default=None)
    mg = sub.add_parser("merge")
    mg.add_argument("files", nargs="+")
    mg.add_argument("--out", required=True)
    a = ap.parse_args()
    (run if a.cmd == "run" else merge)(a)


if __name__ == "__main__":
    main()
