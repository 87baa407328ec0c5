#!/usr/bin/env python3
"""resident_share_ab.py [--n 128] [--sigma 256] [--alternations 5] [--sweep 0-8,16] -- what the resident share of the Sell-64
stream (sb_matrix_resident_share) is worth, measured inside ONE process on ONE placement.

The bench's matrix (HPCG n^3, Sell-64-sigma, kernel mode 0) is uploaded as bench.py uploads it (placement tuner included), then
the clean section-8d loop is timed in windows of 240 bodies (two segments of 120, restarted from x0 = 0 outside the clock, as
bench.py's timed pass), each followed by 120 bodies with the loop's own events around every SpMV launch:
  A/B    windows alternating k = 0 and the rule's k, `alternations` times;
  sweep  one window per k of --sweep, then k = 0 again (drift check).
Prints one JSON object: every window, medians and ranges per k, the A/B gain and the margins it is held against."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparsebench_amd import capi, hostapi  # noqa: E402

SEGMENT, WARM = 120, 20


def parse_sweep(text):
    ks = []
    for part in text.split(","):
        lo, _, hi = part.partition("-")
        ks += list(range(int(lo), int(hi or lo) + 1))
    return ks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--sigma", type=int, default=256)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--sweep", default="0-8,16")
    a = ap.parse_args()
    L = capi.init(0)
    prob = hostapi.Problem("generate", a.n, a.n, a.n, fmt="scs", Cc=64, sigma=a.sigma)
    assert prob.use_packed(0) == 0
    rule = prob.resident_share(-1)
    cg = hostapi.CG(prob)

    def bodies(count, events):
        """`count` loop bodies behind WARM untimed ones: (seconds, mean SpMV us or None)"""
        cg.spmv_timing(False)
        cg.start(itermax=WARM + 2 + count, eps=0.0)
        cg.run_iters(WARM + 1)
        cg.spmv_timing(events)
        L.sb_sync()
        t0 = time.perf_counter()
        cg.run_iters(count)
        L.sb_sync()
        dt = time.perf_counter() - t0
        c = cg.counters()
        cg.finish()
        if c["iters"] != WARM + 1 + count:
            raise RuntimeError("the loop exited early: %r" % c)
        us = None
        if events:
            ms, cnt = cg.spmv_ms()
            us = 1e3 * ms / max(cnt, 1)
            cg.spmv_timing(False)
        return dt, us

    def window(k):
        got = prob.resident_share(k)
        assert got == k, (got, k)
        dt = bodies(SEGMENT, False)[0] + bodies(SEGMENT, False)[0]
        return {"k": k, "us_per_step": 1e6 * dt / (2 * SEGMENT), "spmv_us": bodies(SEGMENT, True)[1]}

    def summary(ws):
        out = {}
        for key in ("us_per_step", "spmv_us"):
            v = [w[key] for w in ws]
            out[key] = {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}
        return out

    window(0), window(rule)  # the device settles under load (the first 50-150 ms after idle time run slower)
    ab = []
    for _ in range(a.alternations):
        ab.append(window(0))
        ab.append(window(rule))
    s0, s1 = summary([w for w in ab if w["k"] == 0]), summary([w for w in ab[1::2]])
    base, new = s0["us_per_step"], s1["us_per_step"]
    gain = 1.0 - new["median"] / base["median"]
    rng0 = (base["max"] - base["min"]) / base["median"]
    sweep = [window(k) for k in parse_sweep(a.sweep)] + [window(0)]
    best = min(sweep, key=lambda w: w["us_per_step"])
    out = {"tool": "resident_share_ab", "library": L.sb_version().decode(), "device": L.sb_device_name().decode(),
           "workload": "hpcg_27pt_%d^3_scs_C64_sigma%d, kernel mode 0, clean loop, windows of %d bodies" % (a.n, a.sigma, 2 * SEGMENT),
           "stream_MB": 12e-6 * prob.nElems, "placement": prob.placement_report(), "rule_k": rule,
           "ab": {"k0": s0, "rule": s1 if rule else None, "gain": gain, "range_of_k0_windows": rng0,
                  "gain_needed": max(0.03, 2.0 * rng0), "is_a_gain": bool(rule) and gain > max(0.03, 2.0 * rng0), "windows": ab},
           "sweep": {"windows": sweep, "fastest_k": best["k"]}}
    print(json.dumps(out))
    cg.free()
    prob.free()


if __name__ == "__main__":
    main()
