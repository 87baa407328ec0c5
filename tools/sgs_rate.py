#!/usr/bin/env python3
"""SGS-preconditioned CG on one GPU against Jacobi PCG IN THE SAME PROCESS, on one problem.

    tools/sgs_rate.py run [--n 128] [--scaled 64] [--nodes 80] [--bodies 100] [--repeats 3] --out one_process.json
    tools/sgs_rate.py merge p1.json p2.json p3.json --out profiles/sgs_rate.json

`run` (one fresh process) creates a Jacobi and an SGS handle per problem -- HPCG n^3 in Sell-64-256 in both kernel modes (5: the
masked row programs, 0: the reference-layout stream), the scaled stencil S A S of scaled^3 and the irregular stand-in of nodes^3
nodes, both Sell-64-256 in the mode the upload selects -- and reports for each
  - nC and the set-up seconds of the SGS handle (the matrix download, the host pass, the upload of the sweep structure);
  - us per loop body of each handle (alternating windows of `bodies` bodies at eps = 0, timed on the device between the end of
    the prologue and the last body) and their ratio;
  - the byte model's ratio: (PCG body bytes - the 16 B/row of z and dinv in the fused r update + sb_pcg_precond_bytes + the
    16 B/row of the r.z pass) / PCG body bytes.  A model, not a measurement;
  - the apply alone: us, and GB/s of sb_pcg_precond_bytes; beside it the matrix's own SpMV in the selected mode, us and GB/s of
    sb_matrix_stream_bytes (what that kernel moves): the project's yardstick for a pass over the matrix;
  - the loop time to eps = 1e-10 ||b|| of both handles with their k (the solve first runs in pieces to find k, then is timed
    with itermax = k: exactly the bodies that reach eps).
Nothing is gated: the tool says what SGS costs and what it buys.  `merge` keeps every process's figures side by side.
"""
import os
import sys
import tempfile
import time

import ratelib
from ratelib import hostapi

PCG_VECTOR_BYTES_PER_ROW = 80.0  # 40 in the p update, 40 in the r update with z
FUSED_Z_BYTES_PER_ROW = 16.0     # of those: dinv read, z written
RZ_PASS_BYTES_PER_ROW = 16.0     # dot_l1_k reads r and z
NOTE = ("one entry per fresh process; only ratios taken inside one process count (DESIGN 4.1).  Nothing is gated: "
        "the figures say what an SGS body costs against a Jacobi body and what it buys in iterations")


def measure(L, a, label, p, mode):
    if mode is not None and p.use_packed(mode) != mode:
        raise RuntimeError("%s has no kernel mode %d" % (label, mode))
    t0 = time.perf_counter()
    solvers = {"jacobi": hostapi.PCG(p)}
    t1 = time.perf_counter()
    solvers["sgs"] = hostapi.PCG(p, precond="sgs")
    t2 = time.perf_counter()
    sgs = solvers["sgs"]
    n = p.nr
    bodies = a.bodies
    us = ratelib.body_windows(solvers, list(solvers), bodies, a.repeats)
    med = ratelib.medians(us)
    pcg_model = L.sb_matrix_spmv_bytes(p.matrix) + PCG_VECTOR_BYTES_PER_ROW * n
    sgs_model = pcg_model - FUSED_Z_BYTES_PER_ROW * n + sgs.precond_bytes() + RZ_PASS_BYTES_PER_ROW * n
    apply_us = {name: 1e3 * s.apply_ms(a.apply_reps) for name, s in solvers.items()}
    mv_us = ratelib.spmv_us(L, p, a.apply_reps)
    eps = ratelib.rel_eps(p)
    ks = ratelib.find_ks(solvers, a, eps)
    ms = ratelib.to_eps_rounds(solvers, ks, eps, a.repeats if all(ratelib.reached(ks, a.itermax).values()) else 0)
    mmed = ratelib.medians(ms)
    out = {"problem": label, "rows": n, "kernel_mode": p.pack_info()["mode"], "nC": sgs.colours(),
           "setup_seconds": {"jacobi": round(t1 - t0, 3), "sgs": round(t2 - t1, 3)},
           "launches_per_body": {name: s.launches_per_body() for name, s in solvers.items()},
           "bodies_per_window": bodies,
           "us_per_body": ratelib.rounded(us, 2), "us_per_body_median": ratelib.rounded(med, 2),
           "sgs_over_jacobi_body": round(med["sgs"] / med["jacobi"], 4),
           "model_bytes_per_body": {"jacobi": int(pcg_model), "sgs": int(sgs_model)},
           "model_ratio": round(sgs_model / pcg_model, 4),
           "precond_bytes": {name: int(s.precond_bytes()) for name, s in solvers.items()},
           "apply_us": {name: round(v, 2) for name, v in apply_us.items()},
           "apply_GBps": {name: round(s.precond_bytes() / (1e3 * apply_us[name]), 1) for name, s in solvers.items()},
           "spmv_us": round(mv_us, 2), "spmv_stream_bytes": int(p.stream_bytes()),
           "spmv_GBps": round(p.stream_bytes() / (1e3 * mv_us), 1),
           "eps_rel": 1e-10, "k": ks,
           "loop_ms_to_eps": ratelib.rounded(ms, 3), "loop_ms_to_eps_median": ratelib.rounded(mmed, 3),
           "sgs_over_jacobi_time_to_eps": ratelib.ratio(mmed["sgs"], mmed["jacobi"]),
           "sgs_over_jacobi_iterations": round(ks["sgs"] / ks["jacobi"], 4)}
    for s in solvers.values():
        s.free()
    print("measured:", label, file=sys.stderr, flush=True)
    return out


def run(a):
    L = ratelib.capi.init(0)
    out = dict(ratelib.process_header(L), cases=[])
    want = set(a.cases.split(","))
    if "hpcg" in want:
        p = hostapi.Problem("generate", a.n, a.n, a.n, **ratelib.FMT)
        for mode in (5, 0):
            out["cases"].append(measure(L, a, "hpcg%d mode %d" % (a.n, mode), p, mode))
        p.free()
    if "scaled" in want:
        path = ratelib.write_scaled(os.path.join(tempfile.mkdtemp(prefix="sgs_rate_"), "scaled_hpcg_%d.mtx" % a.scaled), a.scaled)
        p = hostapi.Problem(path, 1, 1, 1, **ratelib.FMT)
        out["cases"].append(measure(L, a, "scaled%d" % a.scaled, p, None))
        p.free()
        os.remove(path)
    if "irregular" in want:
        p = hostapi.Problem("irregular", a.nodes, a.nodes, a.nodes, **ratelib.FMT)
        out["cases"].append(measure(L, a, "irregular, %d^3 nodes" % a.nodes, p, None))
        p.free()
    ratelib.emit(out, a.out)


def merge(a):
    ratelib.merge_cases(a, NOTE)


def main(parse=True):
    return ratelib.cli(run, merge, lambda r: r.add_argument("--cases", default="hpcg,scaled,irregular"), parse,
                       n=128, scaled=64, nodes=80, bodies=100, repeats=3, apply_reps=20, itermax=5000, piece=10)


if __name__ == "__main__":
    main()
