#!/usr/bin/env python3
"""Preconditioned CG on N ranks against sb_cg of the SAME processes, on both data planes.

    python -m torch.distributed.run --nnodes=1 --nproc-per-node N tools/pcg_multirank_rate.py [--brick 128] [--bodies 100]
        [--repeats 3] [--transport rccl|host] --out profiles/pcg_multirank_rate.json

Every rank holds the `bench.py --gpus N` brick (brick^3 rows per rank, Sell-64-256) and creates three handles on it: sb_cg, Jacobi
PCG and the polynomial at (3 steps, ratio 16).  For the peer-mapped plane and for the communicator's (sb_comm_data_plane) rank 0
reports
  - us per loop body of each handle: alternating windows of `bodies` bodies at eps = 0, timed on the device between the end of
    the prologue and the last body, the slowest rank's time, the median of `repeats` windows; and the ratios to sb_cg's;
  - the loop time to eps = 1e-10 ||b|| of each handle with its k (the solve is first run to find k, then timed with itermax = k);
  - sb_cg's phase timings of the beta step, beside which the PCG beta step's second exchange can be judged: the difference of
    the two bodies less the byte model's 4 % is what it costs.  A model, not a measurement.
Only ratios inside one process count.  Nothing is gated.  With more ranks than GPUs the ranks' kernels keep each
other off the CUs and wait for each other inside them: the tool then runs (a rehearsal of its own code) and writes
"measured": false and no ratio.
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsebench_amd import hostapi, srchash  # noqa: E402
from sparsebench_amd.bench.context import RankContext  # noqa: E402


def window_us(ctx, s, bodies):
    """us per body of one window of `bodies` bodies at eps = 0: the slowest rank's loop time"""
    ctx.barrier()
    s.start(bodies + 1, 0.0)
    s.run_iters(bodies)
    s.finish()
    return 1e3 * ctx.rank_max(s.loop_ms()) / bodies


def cg_window_us(ctx, cg, bodies):
    ctx.barrier()
    cg.solve(bodies + 1, 0.0)
    return 1e3 * ctx.rank_max(cg.loop_ms()) / bodies


def to_eps(ctx, s, eps, cap):
    """(k, loop ms of exactly the bodies that reach eps)"""
    k = s.solve(cap, eps)
    ctx.barrier()
    s.solve(k, eps)
    return k, ctx.rank_max(s.loop_ms())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--brick", type=int, default=128, help="rows per rank: brick^3")
    ap.add_argument("--bodies", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cap", type=int, default=500, help="itermax of the solves to eps")
    ap.add_argument("--transport", choices=("rccl", "host"), default="rccl")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    a.steps, a.warmup, a.full, a.fused, a.graph, a.fuse_p, a.fuse_alpha, a.fuse_beta = a.bodies, 0, False, 1, 0, -1, -1, -1
    ctx = RankContext(a)
    L, rank, world = ctx.L, ctx.rank, ctx.world
    if world < 2:
        raise SystemExit("pcg_multirank_rate: start it under torch.distributed.run with 2 or more ranks")
    shared = world > max(L.sb_device_count(), 1)
    prob = hostapi.Problem("generate", a.brick, a.brick, a.brick, fmt="scs", Cc=64, sigma=256, rank=rank, size=world)
    cg, jac, poly = ctx.new_cg(prob), hostapi.PCG(prob), hostapi.PCG(prob, precond="poly", steps=3, ratio=16.0)
    import numpy as np
    import torch
    b, _ = prob.rhs()
    bb = torch.tensor([float(np.dot(b, b))], dtype=torch.float64)
    ctx.dist.all_reduce(bb)
    eps = 1e-10 * math.sqrt(float(bb[0]))
    planes = []
    for plane in (1, 0):
        L.sb_comm_data_plane(plane)
        rec = {"data_plane": "peer_mapped" if plane else "communicator", "in_kernel_allreduce": bool(L.sb_comm_p2p_enabled()) and bool(plane),
               "peer_mapped_halo": bool(L.sb_halo_p2p_enabled(prob.halo)) and bool(plane),
               "launches_per_body": {"cg": cg.launches_per_body(), "jacobi": jac.launches_per_body(), "poly_3_16": poly.launches_per_body()},
               "collectives_per_body": {"cg": cg.collectives_per_body(), "jacobi": jac.collectives_per_body(),
                                        "poly_3_16": poly.collectives_per_body()}}
        us = {"cg": [], "jacobi": [], "poly_3_16": []}
        cg_window_us(ctx, cg, 5), window_us(ctx, jac, 5), window_us(ctx, poly, 5)  # untimed: first-launch costs
        for _ in range(a.repeats):  # alternating windows
            us["cg"].append(cg_window_us(ctx, cg, a.bodies))
            us["jacobi"].append(window_us(ctx, jac, a.bodies))
            us["poly_3_16"].append(window_us(ctx, poly, a.bodies))
        med = {k: statistics.median(v) for k, v in us.items()}
        rec["us_per_body_windows"] = {k: [round(x, 3) for x in v] for k, v in us.items()}
        cg.phase_timing(True)
        cg_window_us(ctx, cg, a.bodies)
        rec["cg_phase_us"] = {k: round(v[0], 3) for k, v in cg.phase_us().items()}
        cg.phase_timing(False)
        solves = {}
        for name, s in (("cg", cg), ("jacobi", jac), ("poly_3_16", poly)):
            k, ms = to_eps(ctx, s, eps, a.cap)
            solves[name] = {"k": k, "loop_ms": round(ms, 3)}
        rec["to_eps_1e-10"] = solves
        if not shared:
            rec["us_per_body"] = {k: round(v, 3) for k, v in med.items()}
            rec["body_over_cg"] = {k: round(med[k] / med["cg"], 4) for k in ("jacobi", "poly_3_16")}
            rec["byte_model_jacobi_over_cg"] = 1.04
            rec["jacobi_body_minus_cg_body_us"] = round(med["jacobi"] - med["cg"], 3)
            rec["loop_ms_to_eps_over_cg"] = {k: round(solves[k]["loop_ms"] / solves["cg"]["loop_ms"], 4) for k in ("jacobi", "poly_3_16")}
        planes.append(rec)
    L.sb_comm_data_plane(1)
    out = {"library": ctx.version, "csrc_hash": srchash.csrc_hash(), "ranks": world,
           "gpus": L.sb_device_count(), "rows_per_rank": prob.nr, "brick": "%d^3 per rank, Sell-64-256" % a.brick, "transport": a.transport,
           "measured": not shared,
           "note": ("one process per rank; only the ratios inside one run count (DESIGN 4.1); nothing is gated" if not shared else
                    "UNMEASURED: %d ranks share %d GPU(s); their kernels keep each other off the CUs and wait for each other inside "
                    "them, so the windows below say nothing about ranks with a GPU each and no ratio is formed" % (world, L.sb_device_count())),
           "planes": planes}
    cg.free(), jac.free(), poly.free(), prob.free()
    if rank == 0:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps({k: out[k] for k in ("ranks", "gpus", "measured")}), flush=True)
    ctx.finalize()


if __name__ == "__main__":
    main()
