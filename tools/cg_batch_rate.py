#!/usr/bin/env python3
"""Batched CG on one GPU against the single right-hand-side loop IN THE SAME PROCESS: HPCG 128^3, Sell-64-256, eps = 0.

    tools/cg_batch_rate.py run [--n 128] [--bodies 250] [--repeats 4] --out one_process.json
    tools/cg_batch_rate.py merge p1.json p2.json p3.json --out profiles/cg_batch_rate_hpcg128.json

`run` (one fresh process): a warm-up solve of each variant, then `repeats` solves of `bodies` loop bodies each, the variants
alternating -- the single-RHS streaming loop (hostapi.CG with the reference-layout kernel, use_packed(0): the code that
existed before the batched path did, so it is the yardstick) and the batched loop with 2, 4 and 8 right-hand sides.  Every
solve is timed on the device over its loop bodies (sb_cg_loop_ms / sb_cgb_loop_ms); eps = 0, so every body runs, which is
checked against the device's counters.  Per variant: us per body, us per body and right-hand side, the gain per right-hand
side over the single loop of THIS process, model bytes / time / 8 TB/s, and the SpMMV kernel alone (HIP events around a
batch of launches, sb_matrix_spmmv_bytes).  `merge` keeps every process's figures side by side: between processes the single
loop itself moves by up to 1.24 x with placement, so a gain counts only if it exceeds that in every process.

Byte model of one body: sb_matrix_spmmv_bytes(nv) + nv * 64 B/row (40 in the p update, 24 in the r update).
"""
import json
import statistics

import numpy as np

import ratelib
from ratelib import PEAK, hostapi

DeviceVector = ratelib.capi.DeviceVector
WIDTHS = (2, 4, 8)
PLACEMENT_SPREAD = 1.24  # 141 / 114 us: what the single loop itself moves by between processes
SAME = ("problem", "format", "bodies_per_solve", "repeats", "timed_bodies_per_variant")


def spmmv_alone_us(L, p, nv, launches=40):
    """us per launch of the product with its fused dot, nv = 1: the single-vector streaming kernel"""
    nr, nc = p.nr, p.nc
    nG = (nr + 255) // 256
    x = DeviceVector.from_host(np.full(nc * nv, 0.5))
    y = DeviceVector(nr * nv)
    q = DeviceVector(max(nv * nG, 4 * nG) + 4)

    def launch():
        if nv == 1:
            L.sb_spmv_native_dot(p.matrix, x.ptr, y.ptr, q.ptr)
        else:
            L.sb_spmmv_native_dot(p.matrix, nv, x.ptr, y.ptr, q.ptr)

    for _ in range(5):
        launch()
    a, b = L.sb_event_create(), L.sb_event_create()
    L.sb_event_record(a)
    for _ in range(launches):
        launch()
    L.sb_event_record(b)
    us = 1e3 * L.sb_event_elapsed_ms(a, b) / launches
    L.sb_event_destroy(a), L.sb_event_destroy(b)
    for d in (x, y, q):
        d.free()
    return us


def run(a):
    L = ratelib.capi.init(0)
    n = a.n
    p = hostapi.Problem("generate", n, n, n, **ratelib.FMT)
    assert p.use_packed(0) == 0  # the single loop streams the reference layout, as the batched loop does
    solvers = {1: hostapi.CG(p, dot_order="tree")}
    for nv in WIDTHS:
        solvers[nv] = hostapi.BatchCG(p, nrhs=nv)
    bodies = a.bodies

    def timed(nv):  # (ratelib.window_us with a body counter per right-hand side)
        s = solvers[nv]
        k = s.solve(bodies + 1, 0.0)
        c = s.counters() if nv == 1 else s.counters(0)
        ran = [c["n_pAp"]] if nv == 1 else [s.counters(j)["n_pAp"] for j in range(nv)]
        if k != bodies + 1 or any(v != bodies for v in ran):
            raise RuntimeError("the timed loop did not run every body: nv=%d k=%d bodies run %r" % (nv, k, ran))
        return 1e3 * s.loop_ms() / bodies

    us = ratelib.alternate(list(solvers), a.repeats, timed)
    launches = {1: solvers[1].launches_per_body()}
    launches.update({nv: solvers[nv].launches_per_body() for nv in WIDTHS})
    for s in solvers.values():
        s.free()
    single = statistics.median(us[1])
    out = dict({"problem": "hpcg%d" % n, "format": "Sell-64-256", "bodies_per_solve": bodies, "repeats": a.repeats,
                "timed_bodies_per_variant": bodies * a.repeats}, **ratelib.process_header(L), variants={})
    for nv in solvers:
        model = L.sb_matrix_spmmv_bytes(p.matrix, nv) + nv * 64.0 * p.nr if nv > 1 else L.sb_matrix_spmv_bytes(p.matrix) + 64.0 * p.nr
        med = statistics.median(us[nv])
        k_us = spmmv_alone_us(L, p, nv)
        k_bytes = L.sb_matrix_spmmv_bytes(p.matrix, nv) if nv > 1 else L.sb_matrix_spmv_bytes(p.matrix)
        out["variants"]["nrhs%d" % nv] = {
            "loop": "single-RHS streaming loop (hostapi.CG, use_packed(0))" if nv == 1 else "batched loop",
            "launches_per_body": launches[nv], "us_per_body": [round(v, 2) for v in us[nv]], "us_per_body_median": round(med, 2),
            "us_per_body_and_rhs": round(med / nv, 2), "gain_per_rhs_over_single": round(single / (med / nv), 3),
            "model_bytes_per_body": int(model), "frac_of_8TBs_on_model_bytes": round(model / (med * 1e-6) / PEAK, 4),
            "spmmv_kernel_us": round(k_us, 2), "spmmv_kernel_bytes": int(k_bytes),
            "spmmv_kernel_frac_of_8TBs": round(k_bytes / (k_us * 1e-6) / PEAK, 4)}
    p.free()
    ratelib.emit(out, a.out)


def merge(a):
    runs = ratelib.load_runs(a.files, SAME)
    gains4 = [r["variants"]["nrhs4"]["gain_per_rhs_over_single"] for r in runs]
    note = ("per variant: one entry per fresh process (the median of its repeats); gain = the single loop's us per body of "
            "the SAME process / the variant's us per body and right-hand side; delivers = the gain at nrhs 4 exceeds the "
            "placement spread in every process")
    out = ratelib.merge_head(runs, note, SAME, variants={}, placement_spread_of_the_single_loop=PLACEMENT_SPREAD,
                             delivers=bool(all(g > PLACEMENT_SPREAD for g in gains4)))
    for v in runs[0]["variants"]:
        rows = [r["variants"][v] for r in runs]
        out["variants"][v] = {k: ([r[k] for r in rows] if k not in ("loop", "launches_per_body", "model_bytes_per_body", "spmmv_kernel_bytes")
                                  else rows[0][k]) for k in rows[0]}
    ratelib.dump(out, a.out)
    print(json.dumps(out))


def main(parse=True):
    return ratelib.cli(run, merge, None, parse, n=128, bodies=250, repeats=4)


if __name__ == "__main__":
    main()
