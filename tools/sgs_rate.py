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
import argparse
import json
import math
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsebench_amd import capi, hostapi, srchash  # noqa: E402

PCG_VECTOR_BYTES_PER_ROW = 80.0  # 40 in the p update, 40 in the r update with z
FUSED_Z_BYTES_PER_ROW = 16.0     # of those: dinv read, z written
RZ_PASS_BYTES_PER_ROW = 16.0     # dot_l1_k reads r and z


def write_scaled(path, n):
    """S A S of the generated n^3 stencil, s_i = 2^((i mod 7) - 3), as a `general` Matrix Market file (exact in binary)"""
    p = hostapi.Problem("generate", n, n, n, fmt="crs", upload=False)
    rp = p.array("rowPtr").astype(np.int64)
    col, val = p.gm_entries()
    col = np.asarray(col, dtype=np.int64)
    row = np.repeat(np.arange(p.nr, dtype=np.int64), np.diff(rp))
    s = lambda i: 2.0 ** ((i % 7) - 3)  # noqa: E731
    v = (s(row) * np.asarray(val, dtype=np.float64)) * s(col)
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write("%d %d %d\n" % (p.nr, p.nr, len(v)))
        step = 1 << 20
        for a in range(0, len(v), step):
            f.write("".join("%d %d %.17g\n" % t for t in zip((row[a:a + step] + 1).tolist(), (col[a:a + step] + 1).tolist(), v[a:a + step].tolist())))
    p.free()
    return path


def find_k(s, itermax, eps, piece):
    s.start(itermax, eps)
    done = 0
    while done < itermax - 1:
        s.run_iters(min(piece, itermax - 1 - done))
        done += piece
        if s.counters()["stop"]:
            break
    return s.finish()


def to_eps(s, k, eps):
    got = s.solve(k, eps)
    ran = s.counters()["n_pAp"]
    if got != k or ran != k - 1:
        raise RuntimeError("the timed solve did not run the %d bodies that reach eps: k=%d bodies run %d" % (k - 1, got, ran))
    return s.loop_ms()


def spmv_us(L, p, reps):
    x, y = L.sb_malloc(8 * p.nc + 4096), L.sb_malloc(8 * p.nr + 4096)
    L.sb_memset(x, 0, 8 * p.nc), L.sb_memset(y, 0, 8 * p.nr)
    e0, e1 = L.sb_event_create(), L.sb_event_create()
    for _ in range(3):
        L.sb_spmv_native(p.matrix, x, y)
    L.sb_event_record(e0)
    for _ in range(reps):
        L.sb_spmv_native(p.matrix, x, y)
    L.sb_event_record(e1)
    us = 1e3 * L.sb_event_elapsed_ms(e0, e1) / reps
    L.sb_event_destroy(e0), L.sb_event_destroy(e1), L.sb_free(x), L.sb_free(y)
    return us


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

    def timed(name):
        s = solvers[name]
        k = s.solve(bodies + 1, 0.0)
        ran = s.counters()["n_pAp"]
        if k != bodies + 1 or ran != bodies:
            raise RuntimeError("the timed loop did not run every body: %s k=%d bodies run %d" % (name, k, ran))
        return 1e3 * s.loop_ms() / bodies

    for name in solvers:  # warm-up
        timed(name)
    us = {name: [] for name in solvers}
    for _ in range(a.repeats):
        for name in solvers:
            us[name].append(timed(name))
    med = {name: statistics.median(v) for name, v in us.items()}
    pcg_model = L.sb_matrix_spmv_bytes(p.matrix) + PCG_VECTOR_BYTES_PER_ROW * n
    sgs_model = pcg_model - FUSED_Z_BYTES_PER_ROW * n + sgs.precond_bytes() + RZ_PASS_BYTES_PER_ROW * n
    apply_us = {name: 1e3 * s.apply_ms(a.apply_reps) for name, s in solvers.items()}
    mv_us = spmv_us(L, p, a.apply_reps)
    b = p.rhs()[0]
    eps = 1e-10 * float(np.linalg.norm(b))
    ks = {name: find_k(s, a.itermax, eps, a.piece) for name, s in solvers.items()}
    ms = {name: [] for name in solvers}
    if all(1 < k < a.itermax for k in ks.values()):
        for _ in range(a.repeats):
            for name, s in solvers.items():
                ms[name].append(to_eps(s, ks[name], eps))
    mmed = {name: (statistics.median(v) if v else None) for name, v in ms.items()}
    out = {"problem": label, "rows": n, "kernel_mode": p.pack_info()["mode"], "nC": sgs.colours(),
           "setup_seconds": {"jacobi": round(t1 - t0, 3), "sgs": round(t2 - t1, 3)},
           "launches_per_body": {name: s.launches_per_body() for name, s in solvers.items()},
           "bodies_per_window": bodies,
           "us_per_body": {name: [round(v, 2) for v in vals] for name, vals in us.items()},
           "us_per_body_median": {name: round(v, 2) for name, v in med.items()},
           "sgs_over_jacobi_body": round(med["sgs"] / med["jacobi"], 4),
           "model_bytes_per_body": {"jacobi": int(pcg_model), "sgs": int(sgs_model)},
           "model_ratio": round(sgs_model / pcg_model, 4),
           "precond_bytes": {name: int(s.precond_bytes()) for name, s in solvers.items()},
           "apply_us": {name: round(v, 2) for name, v in apply_us.items()},
           "apply_GBps": {name: round(s.precond_bytes() / (1e3 * apply_us[name]), 1) for name, s in solvers.items()},
           "spmv_us": round(mv_us, 2), "spmv_stream_bytes": int(p.stream_bytes()),
           "spmv_GBps": round(p.stream_bytes() / (1e3 * mv_us), 1),
           "eps_rel": 1e-10, "k": ks,
           "loop_ms_to_eps": {name: [round(v, 3) for v in vals] for name, vals in ms.items()},
           "loop_ms_to_eps_median": {name: (round(v, 3) if v is not None else None) for name, v in mmed.items()},
           "sgs_over_jacobi_time_to_eps": round(mmed["sgs"] / mmed["jacobi"], 4) if mmed["sgs"] and mmed["jacobi"] else None,
           "sgs_over_jacobi_iterations": round(ks["sgs"] / ks["jacobi"], 4)}
    for s in solvers.values():
        s.free()
    print("measured:", label, file=sys.stderr, flush=True)
    return out


def run(a):
    L = capi.init(0)
    out = {"device": L.sb_device_name().decode(), "library": L.sb_version().decode(), "csrc_hash": srchash.csrc_hash(), "cases": []}
    want = set(a.cases.split(","))
    if "hpcg" in want:
        p = hostapi.Problem("generate", a.n, a.n, a.n, fmt="scs", Cc=64, sigma=256)
        for mode in (5, 0):
            out["cases"].append(measure(L, a, "hpcg%d mode %d" % (a.n, mode), p, mode))
        p.free()
    if "scaled" in want:
        path = write_scaled(os.path.join(tempfile.mkdtemp(prefix="sgs_rate_"), "scaled_hpcg_%d.mtx" % a.scaled), a.scaled)
        p = hostapi.Problem(path, 1, 1, 1, fmt="scs", Cc=64, sigma=256)
        out["cases"].append(measure(L, a, "scaled%d" % a.scaled, p, None))
        p.free()
        os.remove(path)
    if "irregular" in want:
        p = hostapi.Problem("irregular", a.nodes, a.nodes, a.nodes, fmt="scs", Cc=64, sigma=256)
        out["cases"].append(measure(L, a, "irregular, %d^3 nodes" % a.nodes, p, None))
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
    out = dict(head, processes=len(runs), devices=sorted({r["device"] for r in runs}),
               note="one entry per fresh process; only ratios taken inside one process count (DESIGN 4.1).  Nothing is gated: "
                    "the figures say what an SGS body costs against a Jacobi body and what it buys in iterations",
               runs=[r["cases"] for r in runs])
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--n", type=int, default=128)
    r.add_argument("--scaled", type=int, default=64)
    r.add_argument("--nodes", type=int, default=80)
    r.add_argument("--cases", default="hpcg,scaled,irregular")
    r.add_argument("--bodies", type=int, default=100)
    r.add_argument("--repeats", type=int, default=3)
    r.add_argument("--apply-reps", dest="apply_reps", type=int, default=20)
    r.add_argument("--itermax", type=int, default=5000)
    r.add_argument("--piece", type=int, default=10)
    r.add_argument("--out", default=None)
    mg = sub.add_parser("merge")
    mg.add_argument("files", nargs="+")
    mg.add_argument("--out", required=True)
    a = ap.parse_args()
    (run if a.cmd == "run" else merge)(a)


if __name__ == "__main__":
    main()
