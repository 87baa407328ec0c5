#!/usr/bin/env python3
"""Single against double precision on one GPU: HPCG 128^3, Sell-64-256 and CRS, the section-8d loop (fused, tree order).

Prints ONE JSON line.  Per (format, precision): ms_per_step of the loop (HIP events around `steps` bodies after `warmup`),
the SpMV's microseconds between HIP events inside the loop (sb_cg_spmv_timing), its algorithmic bytes
(sb_matrix_spmv_bytes: SP SCS 8 B/element + 8 B/chunk + 4 B/padded row + 4 B/column, SP CRS 8 B/nnz + 4 B/(row+1) +
4 B/row + 4 B/column; DP 12 / 8 / 8 / 8) and the fraction of 8 TB/s those bytes reach.  The DP matrices get the
upload's placement tuner (its report is included), the SP ones stream where hipMalloc put them.
Two more rows per format run the structure-exploiting loops in the same process: `..._fp32_mirror` (the opt-in SP mirror,
sb_set_sp_mirror: spmv_prog_fusep_f32, 3 launches per body) and `..._fp64_mirror` (the fp64 default: masked row programs,
spmv_prog_fusep); every row carries `stream_bytes`, what its selected kernel really moves (sb_matrix_stream_bytes).

usage: tools/sp_rate.py [--n 128] [--steps 40] [--warmup 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsebench_amd import capi, hostapi  # noqa: E402

PEAK = 8.0e12


def one(L, n, fmt, Cc, sigma, precision, steps, warmup, mirror=False):
    p = hostapi.Problem("generate", n, n, n, fmt=fmt, Cc=Cc, sigma=sigma, precision=precision,
                        mirror=mirror if precision == "single" else None)
    if mirror:
        if p.use_packed(5) != 5:
            raise RuntimeError("%s %s: no row programs for this matrix" % (fmt, precision))
    elif precision == "double":
        p.use_packed(0)  # the reference layout: the stream the SP matrix has too (the section-8d loop)
    cg = hostapi.CG(p, fused=True, dot_order="tree")
    itermax = warmup + 2 * steps + 10
    cg.start(itermax)
    cg.run_iters(warmup)
    a, b = L.sb_event_create(), L.sb_event_create()
    L.sb_event_record(a)
    cg.run_iters(steps)
    L.sb_event_record(b)
    ms = L.sb_event_elapsed_ms(a, b)
    cg.spmv_timing(True)
    cg.run_iters(steps)
    spmv_ms, launches = cg.spmv_ms()
    cg.spmv_timing(False)
    k = cg.finish()
    L.sb_event_destroy(a), L.sb_event_destroy(b)
    us = 1e3 * spmv_ms / max(launches, 1)
    nbytes = p.spmv_bytes()
    out = {"ms_per_step": round(ms / steps, 4), "spmv_us": round(us, 2), "spmv_launches": launches,
           "spmv_bytes": int(nbytes), "frac_of_8TBs": round(nbytes / (us * 1e-6) / PEAK, 4), "k": k,
           "launches_per_body": cg.launches_per_body(), "fuse_p": cg.fuse_p(), "mode": p.pack_info()["mode"],
           "stream_bytes": int(p.stream_bytes())}
    out["frac_of_8TBs_stream_bytes"] = round(out["stream_bytes"] / (us * 1e-6) / PEAK, 4)  # (moved bytes; not a roofline figure)
    if precision == "double":
        out["placement"] = p.placement_report()
    cg.free()
    p.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    L = capi.init(0)
    res = {"problem": "hpcg%d" % a.n, "gpus": 1, "device": L.sb_device_name().decode(), "steps": a.steps}
    for label, fmt, Cc, sigma in (("scs64_256", "scs", 64, 256), ("crs", "crs", 64, 1)):
        for precision, key in (("single", "fp32"), ("double", "fp64")):
            res["%s_%s" % (label, key)] = one(L, a.n, fmt, Cc, sigma, precision, a.steps, a.warmup)
        for precision, key in (("single", "fp32_mirror"), ("double", "fp64_mirror")):
            res["%s_%s" % (label, key)] = one(L, a.n, fmt, Cc, sigma, precision, a.steps, a.warmup, mirror=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
