#!/usr/bin/env python3
"""Restarted GMRES(30) on one GPU: HPCG 128^3, Sell-64-256, the streaming SpMV kernel (mode 0) and the mirror (mode 5);
the fused kernels (multi-dot, multi-update) against the op list IN THE SAME PROCESS -- the op list consists only of kernels
that existed before GMRES did (one tree dot per h entry, one waxpby-shaped launch per projection), so it is the baseline.

    tools/gmres_rate.py run [--n 128] [--restart 30] [--cycles 20] [--repeats 3] --out one_process.json
    tools/gmres_rate.py merge p1.json p2.json p3.json --out profiles/gmres_rate_hpcg128.json

`run` (one fresh process): per mode a warm-up solve of one cycle, then `repeats` solves of `cycles` full cycles each, the two variants alternating, timed
between sb_gmres_start and sb_gmres_finish with sb_gmres_loop_ms (cycle closes included); eps = 0, so the loop runs every
step (checked against the device's step counter).  `merge` quotes, per mode and variant, the median of each process and
the range over the processes (the placement effect of DESIGN 4.1 moves the same kernel by 10-20 % between processes).

Byte model of one fused step at cycle position j: sb_matrix_stream_bytes + (3 (j + 1) + 7) * 8 n; averaged
over a cycle: stream_bytes + (3 (m + 1) / 2 + 7) * 8 n.  `frac_of_8TBs` = model bytes / measured time / 8 TB/s.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsebench_amd import capi, hostapi, srchash  # noqa: E402

PEAK = 8.0e12


def time_variants(p, m, cycles, repeats):
    """us per step of the fused loop and of the op list, alternating, after a warm-up cycle of each"""
    solvers = {True: hostapi.GMRES(p, restart=m, fused=True), False: hostapi.GMRES(p, restart=m, fused=False)}
    for s in solvers.values():
        s.start(m + 2, 0.0)
        s.run_steps(m)  # warm-up: one full cycle
        s.finish()
    steps = cycles * m
    us = {True: [], False: []}
    for _ in range(repeats):
        for fused, s in solvers.items():
            s.start(steps + 2, 0.0)  # (one more than the steps taken: the last cycle closes inside the timed loop too)
            s.run_steps(steps)
            k = s.finish()
            c = s.counters()
            if k != steps + 1 or c["steps"] != steps or c["cycles"] != cycles:
                raise RuntimeError("the timed loop did not run every step: k=%d counters=%r" % (k, c))
            us[fused].append(1e3 * s.loop_ms() / steps)
    launches = [solvers[True].launches_per_step(j) for j in range(m)]
    for s in solvers.values():
        s.free()
    return us[True], us[False], launches


def run(a):
    L = capi.init(0)
    n, m = a.n, a.restart
    p = hostapi.Problem("generate", n, n, n, fmt="scs", Cc=64, sigma=256)
    out = {"problem": "hpcg%d" % n, "format": "Sell-64-256", "restart": m, "cycles_timed": a.cycles, "repeats": a.repeats,
           "device": L.sb_device_name().decode(), "library": L.sb_version().decode(), "csrc_hash": srchash.csrc_hash(), "modes": {}}
    for mode in (0, 5):
        got = p.use_packed(mode)
        stream = p.stream_bytes()
        model = stream + (3.0 * (m + 1) / 2.0 + 7.0) * 8.0 * p.nr
        fused, oplist, launches = time_variants(p, m, a.cycles, a.repeats)
        f, o = statistics.median(fused), statistics.median(oplist)
        out["modes"]["mode%d" % mode] = {
            "kernel_mode_selected": got, "spmv_stream_bytes": int(stream), "model_bytes_per_step": int(model),
            "fused_us_per_step": [round(v, 2) for v in fused], "oplist_us_per_step": [round(v, 2) for v in oplist],
            "fused_us_per_step_median": round(f, 2), "oplist_us_per_step_median": round(o, 2),
            "oplist_over_fused": round(o / f, 3), "fused_frac_of_8TBs_on_model_bytes": round(model / (f * 1e-6) / PEAK, 4),
            "launches_per_step_mean": round(sum(launches) / len(launches), 2), "launches_per_step": launches}
    p.free()
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


def merge(a):
    runs = [json.load(open(f)) for f in a.files]
    head = {k: runs[0][k] for k in ("problem", "format", "restart", "cycles_timed", "repeats", "library", "csrc_hash")}
    if any({k: r[k] for k in head} != head for r in runs):
        raise SystemExit("the runs do not describe the same build and problem")
    out = dict(head, processes=len(runs), devices=sorted({r["device"] for r in runs}), modes={},
               note="per variant: the median of each fresh process, and the range over the processes")
    for mode in runs[0]["modes"]:
        rows = [r["modes"][mode] for r in runs]
        f = [r["fused_us_per_step_median"] for r in rows]
        o = [r["oplist_us_per_step_median"] for r in rows]
        model = rows[0]["model_bytes_per_step"]
        out["modes"][mode] = {
            "kernel_mode_selected": rows[0]["kernel_mode_selected"], "spmv_stream_bytes": rows[0]["spmv_stream_bytes"],
            "model_bytes_per_step": model, "fused_us_per_step": f, "oplist_us_per_step": o,
            "fused_us_per_step_range": [min(f), max(f)], "oplist_us_per_step_range": [min(o), max(o)],
            "oplist_over_fused": [r["oplist_over_fused"] for r in rows],
            "fused_frac_of_8TBs_on_model_bytes": [round(model / (v * 1e-6) / PEAK, 4) for v in f],
            "launches_per_step_mean": rows[0]["launches_per_step_mean"], "launches_per_step": rows[0]["launches_per_step"],
            "all_repeats_fused_us": [r["fused_us_per_step"] for r in rows], "all_repeats_oplist_us": [r["oplist_us_per_step"] for r in rows]}
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--n", type=int, default=128)
    r.add_argument("--restart", type=int, default=30)
    r.add_argument("--cycles", type=int, default=20)
    r.add_argument("--repeats", type=int, default=3)
    r.add_argument("--out", default=None)
    mg = sub.add_parser("merge")
    mg.add_argument("files", nargs="+")
    mg.add_argument("--out", required=True)
    a = ap.parse_args()
    (run if a.cmd == "run" else merge)(a)


if __name__ == "__main__":
    main()
