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
import json
import statistics

import ratelib
from ratelib import PEAK, hostapi

SAME = ("problem", "format", "restart", "cycles_timed", "repeats")


def time_variants(p, m, cycles, repeats):
    """us per step of the fused loop and of the op list, alternating, after a warm-up cycle of each"""
    solvers = {True: hostapi.GMRES(p, restart=m, fused=True), False: hostapi.GMRES(p, restart=m, fused=False)}
    steps = cycles * m

    def warm(fused):
        s = solvers[fused]
        s.start(m + 2, 0.0)
        s.run_steps(m)  # one full cycle
        s.finish()

    def timed(fused):
        s = solvers[fused]
        s.start(steps + 2, 0.0)  # (one more than the steps taken: the last cycle closes inside the timed loop too)
        s.run_steps(steps)
        k = s.finish()
        c = s.counters()
        if k != steps + 1 or c["steps"] != steps or c["cycles"] != cycles:
            raise RuntimeError("the timed loop did not run every step: k=%d counters=%r" % (k, c))
        return 1e3 * s.loop_ms() / steps

    us = ratelib.alternate(list(solvers), repeats, timed, warm)
    launches = [solvers[True].launches_per_step(j) for j in range(m)]
    for s in solvers.values():
        s.free()
    return us[True], us[False], launches


def run(a):
    L = ratelib.capi.init(0)
    n, m = a.n, a.restart
    p = hostapi.Problem("generate", n, n, n, **ratelib.FMT)
    out = dict({"problem": "hpcg%d" % n, "format": "Sell-64-256", "restart": m, "cycles_timed": a.cycles, "repeats": a.repeats},
               **ratelib.process_header(L), modes={})
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
    ratelib.emit(out, a.out)


def merge(a):
    runs = ratelib.load_runs(a.files, SAME)
    out = ratelib.merge_head(runs, "per variant: the median of each fresh process, and the range over the processes", SAME, modes={})
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
    ratelib.dump(out, a.out)
    print(json.dumps(out))


def main(parse=True):
    return ratelib.cli(run, merge, None, parse, n=128, restart=30, cycles=20, repeats=3)


if __name__ == "__main__":
    main()
