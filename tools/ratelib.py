"""What the rate tools (tools/*_rate.py with a `run` and a `merge`) share: plain functions, one definition each.

A tool keeps what is its own -- which handles it makes, the names it gives them, the dictionary it emits -- and takes from here
  - the solves: find_k / to_eps (k in pieces, then one timed solve of exactly the k - 1 bodies), window_us (one window of bodies
    at eps = 0), and the loops around them: alternate (warm every name once, then rounds that alternate over the names) and
    to_eps_rounds; medians and the roundings of what they return;
  - the problems: FMT, rel_eps, spmv_us, write_scaled, write_convdiff, and the four hierarchies spelled out level by level
    (regenerated, galerkin_levels, device_levels, aggregation_levels) with their free;
  - the ends of `run` (process_header, save, emit) and of `merge` (load_runs, merge_head, collect / ranges, dump, merge_cases);
  - the command line (cli).
The order of the GPU work inside every function is part of what the committed profiles mean: it is not to be improved here.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsebench_amd import capi, hostapi, srchash  # noqa: E402,F401  (the tools take capi and hostapi from here)

PEAK = 8.0e12  # B/s
FMT = dict(fmt="scs", Cc=64, sigma=256)
BODIES = {"bicgstab": "n_rv", "cg": "n_pAp", "pcg": "n_pAp", "gmres": "steps"}  # the counter that counts a kind's bodies


# ---- the solves ----------------------------------------------------------------------------------------------------------

def kind(s):
    """bicgstab, cg, pcg or gmres: the handle's class says which"""
    return type(s).__name__.lower()


def find_k(s, itermax, eps, piece):
    """k at which the loop reaches eps (untimed; doubles as the warm-up solve): the solve in pieces, the stop flag read between
    them, so that a converged loop is not followed by thousands of no-op launches.  A handle with run_steps (GMRES) steps"""
    s.start(itermax, eps)
    run = s.run_steps if hasattr(s, "run_steps") else s.run_iters
    done = 0
    while done < itermax - 1:
        cnt = min(piece, itermax - 1 - done)
        run(cnt)
        done += cnt
        if s.counters()["stop"]:
            break
    return s.finish()


def to_eps(s, k, eps, named=False):
    """loop_ms of the k - 1 bodies (steps) that reach eps: one blocking solve with itermax = k, which enqueues exactly those and
    is timed on the device by the solver itself (no-op bodies and host polls would otherwise sit inside the interval)"""
    got = s.solve(k, eps)
    ran = s.counters()[BODIES[kind(s)]]
    if got != k or ran != k - 1:
        who = "%s " % kind(s) if named else ""
        raise RuntimeError("the timed solve did not run the %d bodies that reach eps: %sk=%d bodies run %d" % (k - 1, who, got, ran))
    return s.loop_ms()


def window_us(s, bodies, name):
    """us per body of one window: `bodies` bodies at eps = 0, timed on the device between the prologue's end and the last body"""
    k = s.solve(bodies + 1, 0.0)
    ran = s.counters()[BODIES[kind(s)]]
    if k != bodies + 1 or ran != bodies:
        raise RuntimeError("the timed loop did not run every body: %s k=%d bodies run %d" % (name, k, ran))
    return 1e3 * s.loop_ms() / bodies


def alternate(names, repeats, timed, warm=None):
    """warm every name once, then `repeats` rounds that alternate over the names: name -> [what timed(name) returned]"""
    for name in names:
        (warm or timed)(name)
    out = {name: [] for name in names}
    for _ in range(repeats):
        for name in names:
            out[name].append(timed(name))
    return out


def body_windows(solvers, names, bodies, repeats):
    """alternate() over window_us: name -> [us per body]"""
    return alternate(names, repeats, lambda name: window_us(solvers[name], bodies, name))


def find_ks(solvers, a, eps):
    return {name: find_k(s, a.itermax, eps, a.piece) for name, s in solvers.items()}


def reached(ks, itermax):
    return {name: 1 < k < itermax for name, k in ks.items()}


def to_eps_rounds(solvers, ks, eps, repeats, reached=None, named=False):
    """`repeats` rounds that alternate over the handles, one timed solve to eps each: name -> [loop ms].  Where `reached` is given, a
    name it holds false for is not solved and keeps an empty list"""
    ms = {name: [] for name in solvers}
    for _ in range(repeats):
        for name, s in solvers.items():
            if reached is None or reached[name]:
                ms[name].append(to_eps(s, ks[name], eps, named))
    return ms


def medians(d):
    return {name: (statistics.median(v) if v else None) for name, v in d.items()}


def rounded(d, digits):
    """name -> value or [values], rounded; None stays"""
    r = lambda v: None if v is None else round(v, digits)  # noqa: E731
    return {name: ([r(x) for x in v] if isinstance(v, list) else r(v)) for name, v in d.items()}


def ratio(x, y):
    return round(x / y, 4) if x and y else None


# ---- the problems --------------------------------------------------------------------------------------------------------

def rel_eps(p):
    """1e-10 ||b||"""
    return 1e-10 * float(np.linalg.norm(p.rhs()[0]))


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


def write_convdiff(path, n):
    """7-point upwind convection-diffusion on an n^3 grid: diagonal 6, the three lower neighbours -1.5, the three upper
    neighbours -0.5 (every value exact in binary), as a `general` Matrix Market file; b = 1 by the file rule"""
    idx = np.arange(n ** 3, dtype=np.int64)
    x, y, z = idx % n, (idx // n) % n, idx // (n * n)
    rows, cols, vals = [idx], [idx], [np.full(idx.shape, 6.0)]
    for coord, step in ((x, 1), (y, n), (z, n * n)):
        lo, hi = idx[coord > 0], idx[coord < n - 1]
        rows += [lo, hi]
        cols += [lo - step, hi + step]
        vals += [np.full(lo.shape, -1.5), np.full(hi.shape, -0.5)]
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((c, r))
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write("%d %d %d\n" % (n ** 3, n ** 3, len(r)))
        np.savetxt(f, np.column_stack((r[order] + 1, c[order] + 1, v[order])), fmt="%d %d %.1f")
    return path


def regenerated(p, nlev):
    """the hierarchy PCG(precond="mgpoly", levels=...) makes for itself, made here so that its levels' kernel modes can be set"""
    dims, out = p.dims, []
    for _ in range(nlev - 1):
        P = hostapi.mg_trilinear(*dims)
        dims = tuple(d // 2 for d in dims)
        out.append((hostapi.Problem("generate", *dims, fmt=p.fmt, Cc=p.Cc, sigma=p.sigma_arg), P, 0.25))
    return out


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


def stored(q):
    return q.nnzTrue if q.fmt == "crs" else q.nElems


def device_levels(p, nlev):
    """mg_galerkin(product="device") spelled out, to time its parts per level"""
    dims, fine, out, rows = p.dims, p, [], []
    for l in range(nlev - 1):
        P = hostapi.mg_trilinear(*dims)
        dims = tuple(d // 2 for d in dims)
        nc = dims[0] * dims[1] * dims[2]
        t0 = time.perf_counter()
        (ptr, col, val), st = hostapi.galerkin_product(fine, P, n_coarse=nc)
        t1 = time.perf_counter()
        q = hostapi.Problem.from_csr(ptr, col, val, fmt=p.fmt, Cc=p.Cc, sigma=p.sigma_arg)
        t2 = time.perf_counter()
        n, nnz_p, raw = fine.nr, len(P[1]), len(col) + st["dropped"]
        b1 = 2 * (12.0 * stored(fine) + 12.0 * nnz_p + 8.0 * n) + 12.0 * st["t_entries"] + 8.0 * n
        b2 = 2 * (12.0 * nnz_p + 8.0 * nc + 12.0 * st["t_entries"] + 8.0 * n) + 12.0 * raw + 8.0 * nc
        rows.append({"level": l + 1, "rows": nc, "nnz": len(col), "t_entries": st["t_entries"], "dropped": st["dropped"],
                     "max_row_t": st["max_row_t"], "max_row_ac": st["max_row_ac"],
                     "stage1_ms": round(st["stage1_ms"], 3), "stage2_ms": round(st["stage2_ms"], 3),
                     "product_host_ms": round(1e3 * (t1 - t0) - st["stage1_ms"] - st["stage2_ms"], 3),
                     "convert_upload_ms": round(1e3 * (t2 - t1), 3),
                     "stage1_model_bytes": int(b1), "stage2_model_bytes": int(b2),
                     "stage1_fraction_of_8TBps": round(b1 / (1e-3 * st["stage1_ms"] * PEAK), 4),
                     "stage2_fraction_of_8TBps": round(b2 / (1e-3 * st["stage2_ms"] * PEAK), 4)})
        out.append((q, P, 1.0))
        fine = q
    return out, rows


def aggregation_levels(p):
    """mg_aggregation spelled out, to time its parts per level"""
    fine, out, rows = p, [], []
    while len(out) + 1 < hostapi.MG_AGGREGATION_DEPTH and fine.nr > hostapi.MG_AGGREGATION_COARSEST:
        t0 = time.perf_counter()
        P, n_agg, st = hostapi.sa_prolongation(fine, stats=True)
        t1 = time.perf_counter()
        if 2 * n_agg > fine.nr:
            raise SystemExit("level %d: %d aggregates of %d rows: coarsens by less than 2" % (len(out), n_agg, fine.nr))
        (ptr, col, val), gst = hostapi.galerkin_product(fine, P, n_coarse=n_agg)
        t2 = time.perf_counter()
        q = hostapi.Problem.from_csr(ptr, col, val, fmt=p.fmt, Cc=p.Cc, sigma=p.sigma_arg)
        t3 = time.perf_counter()
        n, e = fine.nr, st["strong_entries"]
        model = st["rounds"] * 2 * (12.0 * e + 16.0 * n + 4.0 * (n + 1))
        dev = st["aggregate_ms"] + st["product_ms"] + st["smooth_ms"]
        rows.append({"level": len(out), "rows": n, "aggregates": n_agg, "rounds": st["rounds"], "strong_entries": e,
                     "nnz_p": len(P[1]), "max_row_p": st["max_row_p"], "max_row_at": gst["max_row_t"], "max_row_ac": gst["max_row_ac"],
                     "nnz_ac": len(col), "aggregate_ms": round(st["aggregate_ms"], 3), "product_ms": round(st["product_ms"], 3),
                     "smooth_ms": round(st["smooth_ms"], 3), "prolongation_host_ms": round(1e3 * (t1 - t0) - dev, 3),
                     "galerkin_stage_ms": round(gst["stage1_ms"] + gst["stage2_ms"], 3),
                     "galerkin_host_ms": round(1e3 * (t2 - t1) - gst["stage1_ms"] - gst["stage2_ms"], 3),
                     "convert_upload_ms": round(1e3 * (t3 - t2), 3), "rounds_model_bytes": int(model),
                     "aggregate_fraction_of_8TBps": round(model / (1e-3 * st["aggregate_ms"] * PEAK), 4)})
        out.append((q, P, 1.0))
        fine = q
    return out, rows


def free(coarse):
    for q, _, _ in coarse:
        q.free()


# ---- the end of `run` ----------------------------------------------------------------------------------------------------

def process_header(L):
    return {"device": L.sb_device_name().decode(), "library": L.sb_version().decode(), "csrc_hash": srchash.csrc_hash()}


def save(out, path):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(out) + "\n")


def emit(out, path):
    print(json.dumps(out))
    save(out, path)


# ---- `merge` -------------------------------------------------------------------------------------------------------------

def load_runs(files, same=()):
    """the per-process files; refused unless all describe one build (and agree on the keys of `same`)"""
    runs = [json.load(open(f)) for f in files]
    keys = tuple(same) + ("library", "csrc_hash")
    if any({k: r[k] for k in keys} != {k: runs[0][k] for k in keys} for r in runs):
        raise SystemExit("the runs do not describe the same build" + (" and problem" if same else ""))
    return runs


def merge_head(runs, note, same=(), **between):
    """what every merged file opens with; `between` goes in front of the note"""
    head = {k: runs[0][k] for k in tuple(same) + ("library", "csrc_hash")}
    return dict(head, processes=len(runs), devices=sorted({r["device"] for r in runs}), **between, note=note)


def collect(rows, name, e, keys):
    """one process's entry `e` into the slot of its name: k must agree, the values of `keys` it holds are appended"""
    slot = rows.setdefault(name, dict({"k": e["k"]}, **{key: [] for key in keys}))
    if e["k"] != slot["k"]:
        raise SystemExit("k of %s differs between processes" % name)
    for key in keys:
        if key in e:
            slot[key].append(e[key])


def ranges(slots, keys):
    """every slot's collected values to [min, max], or None where no process gave one"""
    for slot in slots:
        for key in keys:
            slot[key] = [min(slot[key]), max(slot[key])] if slot[key] else None


def dump(out, path):
    with open(path, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")


def merge_cases(a, note):
    """the merge that keeps every process's cases side by side under `runs`"""
    runs = load_runs(a.files)
    out = dict(merge_head(runs, note), runs=[r["cases"] for r in runs])
    dump(out, a.out)
    print(json.dumps(out))
    return runs


# ---- the command line ----------------------------------------------------------------------------------------------------

def cli(run, merge, add_run_args=None, parse=True, also=None, **ints):
    """`run` with --out, an int option --<name> per keyword (apply_reps: --apply-reps) with its default and what add_run_args
    adds; `merge files... --out`; a further subcommand per entry name -> (function, its add-arguments) of `also`.  Parses and
    dispatches, or returns the parser where parse is false"""
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    for name, default in ints.items():
        r.add_argument("--" + name.replace("_", "-"), dest=name, type=int, default=default)
    if add_run_args:
        add_run_args(r)
    r.add_argument("--out", default=None)
    todo = {"run": run, "merge": merge}
    for name, (fn, add) in (also or {}).items():
        add(sub.add_parser(name))
        todo[name] = fn
    mg = sub.add_parser("merge")
    mg.add_argument("files", nargs="+")
    mg.add_argument("--out", required=True)
    if not parse:
        return ap
    a = ap.parse_args()
    todo[a.cmd](a)
