"""The reference-shaped C API on vectors from allocate() at the sizes where the hook hands out memory that lives in HBM
(host/sbh_base.c: requests of 64 KiB and more).  tests/c/hook_driver.c fills such vectors by host loops, runs spMVM / waxpby /
ddot on them in place with K kernels queued ahead of each checked call, reads every output through the host mapping and
refills inputs; every printed value is compared bit for bit: double against the oracle (oracle/pyoracle.py), single against
tests/sp_ref.py.

The driver runs in its `sync` mode: it calls sbh_profile_sync() after each checked call, before the host touches a vector,
which is what spMVM / waxpby on hook vectors ask of their caller.  Without that mode it is the reference-shaped caller that
never synchronises; measured once on the MI355X at 19x21x23, CRS, K = 64, it read the NaN sentinel in 134 of 9 177 values of
step 3 (rows 9 043 and up, the ones the kernel writes last), in 115 of step 4 and in 7 of step 6.  Making those calls wait
for their kernels cured that (all of this file's cases then passed without `sync`), but it put the launch latency of an idle
stream into the PROFILE region of a kernel that takes 18 us at 128^3: test_reference_spmv_mode_times_the_kernel_not_pcie
then saw its profiler row 11 % to 24 % above the kernel row (3 % to 7 % before), over its 15 %.  So the wait is not in the
library, and the assertions that need it -- the same values WITHOUT `sync` -- are not in this file."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import sp_ref
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")

# the smallest shapes at which the hook is live: one below the 64 KiB threshold, one exactly on it, one above it with a row
# count that is no multiple of 64 or 256 (a partial last chunk and, under sigma = 128, a real permutation)
SHAPES = {"double": {"below": (16, 16, 31), "at": (16, 16, 32), "above": (19, 21, 23)},
          "single": {"below": (16, 32, 31), "at": (16, 32, 32), "above": (23, 27, 29)}}
DTYPE = {"double": np.float64, "single": np.float32}
VECTORS = ("x", "y", "y2", "w")
STEPS = ("s3", "s4", "s5", "s6", "s7w", "s7x", "s9a", "s9b", "s9c")


@functools.lru_cache(maxsize=None)
def build_driver(fmt, precision):
    """tests/c/hook_driver.c the way test_gpu_dropin.build_driver builds dropin_driver.c; single: -DPRECISION=1, the _sp libraries"""
    outdir = tempfile.mkdtemp(prefix="hook_driver_")
    atexit.register(shutil.rmtree, outdir, ignore_errors=True)
    sp = precision == "single"
    exe = os.path.join(outdir, "hook_driver_%s_%s" % (fmt, precision))
    cmd = ["gcc", "-std=gnu11", "-O1", "-Wall", "-D" + fmt] + (["-DPRECISION=1"] if sp else []) + \
          ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "hook_driver.c"), "-o", exe, "-L" + LIB,
           "-lsparsebench_%s%s" % (fmt.lower(), "_sp" if sp else ""), "-lsparsebench_host%s" % ("_sp" if sp else ""),
           "-lsbhip", "-Wl,-rpath," + LIB, "-lm"]
    subprocess.check_call(cmd)
    return exe


_crashed = []  # a driver run that ended on a signal: nothing more is started on the GPU from here


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


@functools.lru_cache(maxsize=None)
def run_driver(fmt, precision, shape, K, mixed=True, allocate_host=False):
    """one run of the driver, parsed: kinds per vector, one array per step, the two dots, the copy counters, the hook's reason"""
    assert not _crashed, "an earlier driver run ended on a signal: %r" % (_crashed,)
    env = dict(os.environ, SB_COPY_REPORT="1")
    env.pop("SPARSEBENCH_ALLOCATE", None)
    if allocate_host:
        env["SPARSEBENCH_ALLOCATE"] = "host"
    args = [build_driver(fmt, precision)] + [str(v) for v in shape] + [str(K), "sync"] + ([] if mixed else ["nomixed"])
    out = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    err = out.stderr.decode()
    if out.returncode < 0:
        _crashed.append((args[1:], out.returncode))
    assert out.returncode == 0, (out.returncode, err[-2000:])
    dt = DTYPE[precision]
    r = {"kinds": {}, "steps": {}}
    cols = {}
    for line in out.stdout.decode().splitlines():
        f = line.split()
        if f[0] == "kind":
            r["kinds"][f[1]] = int(f[2])
        elif f[0] == "dot":
            r["dot"] = np.array([float.fromhex(f[1]), float.fromhex(f[2])]).astype(dt)
        elif f[0] in STEPS:
            cols.setdefault(f[0], []).append((int(f[1]), float.fromhex(f[2])))
    for tag, rows in cols.items():
        assert [i for i, _ in rows] == list(range(len(rows))), tag
        r["steps"][tag] = np.array([v for _, v in rows]).astype(dt)  # (%a of a float is exact in double: the cast restores it)
    c = re.search(r"sbhip copies: h2d (\d+) calls (\d+) bytes, d2h (\d+) calls (\d+) bytes; allocate\(\): last kind (\d) \((.*)\)", err)
    assert c, err[-2000:]
    r["copies"] = [int(c.group(i)) for i in (1, 2, 3, 4)]
    r["reason"] = c.group(6)
    return r


@functools.lru_cache(maxsize=None)
def reference(precision, shape):
    """what the driver's sequence gives in the reference's arithmetic, computed once per shape: {step: array}, (dot, dot), nr"""
    nx, ny, nz = shape
    if precision == "double":
        g = po.GMatrix.generate(nx, ny, nz)
        nr, nc, dt = g.nr, g.nc, np.float64
        spmv, waxpby, dot = g.spmv, po.waxpby, po.ddot_tree
    else:
        from sparsebench_amd import hostapi
        p = hostapi.Problem("generate", nx, ny, nz, fmt="crs", precision="single", upload=False)
        nr, nc, dt = p.nr, p.nc, np.float32
        rp, col, val = p.array("rowPtr").copy(), p.array("crs_colInd").copy(), p.values().copy()
        p.free()
        spmv, waxpby, dot = (lambda v: sp_ref.spmv_crs(rp, col, val, v)), sp_ref.waxpby, sp_ref.dot_tree
    assert nr == nx * ny * nz and nc == nr  # one rank: no external columns
    i = np.arange(nc)
    xa = (1.0 + 0.001 * (i % 97)).astype(dt)  # the driver's fill_a / fill_b: computed in double, stored to CG_FLOAT
    xb = (2.0 - 0.003 * (i % 89)).astype(dt)
    s = {}
    s["s3"] = s["s4"] = spmv(xa)
    y = s["s5"] = spmv(xb)
    s["s6"] = waxpby(1.0, y, -0.5, xb)
    w = s["s7w"] = waxpby(2.0, s["s6"], 1.0, y)
    x = s["s7x"] = waxpby(1.0, xb, -2.0, y)
    dots = np.array([dot(w, y), dot(y, y)]).astype(dt)
    s["s9a"] = spmv(x)
    y = s["s9b"] = spmv(xa)
    s["s9c"] = waxpby(1.0, xa, -0.5, y)
    return {k: np.ascontiguousarray(v, dtype=dt) for k, v in s.items()}, dots, nr


def check_values(r, precision, shape, steps=STEPS):
    ref, dots, nr = reference(precision, shape)
    for tag in steps:
        got = r["steps"][tag]
        assert got.shape == (nr,), (tag, got.shape)
        bad = np.nonzero(np.isnan(got))[0]
        assert bad.size == 0, "%s: %d of %d values are the NaN sentinel, e.g. rows %s" % (tag, bad.size, nr, bad[-5:])
        assert same_bits(got, ref[tag]), (tag, np.nonzero(got != ref[tag])[0][:5])
    assert not np.isnan(r["dot"]).any() and same_bits(r["dot"], dots), (r["dot"], dots)


@pytest.mark.parametrize("K", [8, 64])
@pytest.mark.parametrize("where", ["below", "at", "above"])
@pytest.mark.parametrize("precision", ["double", "single"])
@pytest.mark.parametrize("fmt", ["CRS", "SCS"])
def test_hook_vectors_give_the_references_bits(gpu, fmt, precision, where, K):
    """steps 3-9 of hook_driver.c: no sentinel anywhere, every value the reference's, with K kernels queued ahead"""
    shape = SHAPES[precision][where]
    r = run_driver(fmt, precision, shape, K)
    want = 0 if where == "below" else 1
    if want == 1 and set(r["kinds"].values()) != {1}:
        pytest.skip("no host-visible device memory on this box: %s" % r["reason"])
    assert r["kinds"] == {v: want for v in VECTORS}, r["kinds"]
    check_values(r, precision, shape)


@pytest.mark.parametrize("precision", ["double", "single"])
@pytest.mark.parametrize("fmt", ["CRS", "SCS"])
def test_hook_vectors_are_not_staged(gpu, fmt, precision):
    """nothing is staged for a hook vector however many calls are made; each mixed call of step 9 stages its one plain vector"""
    shape = SHAPES[precision]["above"]
    r8, r64, r8n = (run_driver(fmt, precision, shape, K, mixed) for K, mixed in ((8, True), (64, True), (8, False)))
    if set(r8["kinds"].values()) != {1}:
        pytest.skip("no host-visible device memory on this box: %s" % r8["reason"])
    assert r8["copies"] == r64["copies"], (r8["copies"], r64["copies"])
    check_values(r8n, precision, shape, steps=STEPS[:6])
    nr = reference(precision, shape)[2]
    vec = nr * np.dtype(DTYPE[precision]).itemsize
    # step 9: spMVM(hook x, plain y) copies y out; spMVM(plain x, hook y) and waxpby(plain x, hook y, hook w) copy x in
    assert [a - b for a, b in zip(r8["copies"], r8n["copies"])] == [2, 2 * vec, 1, vec], (r8["copies"], r8n["copies"])


@pytest.mark.parametrize("precision", ["double", "single"])
@pytest.mark.parametrize("fmt", ["CRS", "SCS"])
def test_plain_host_allocation_gives_the_same_bits(gpu, fmt, precision):
    """SPARSEBENCH_ALLOCATE=host: the same driver on plain host vectors (kind 0, staged per call), the same bits"""
    shape = SHAPES[precision]["above"]
    r = run_driver(fmt, precision, shape, 8, allocate_host=True)
    assert r["kinds"] == {v: 0 for v in VECTORS}, r["kinds"]
    check_values(r, precision, shape)


@pytest.mark.parametrize("precision", ["double", "single"])
def test_allocation_table_grows_past_256_blocks(gpu, precision):
    """300 live requests of 64 KiB: each is device memory while held and all of it comes back on release"""
    env = dict(os.environ)
    env.pop("SPARSEBENCH_ALLOCATE", None)
    out = subprocess.run([build_driver("CRS", precision), "table"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    txt = out.stdout.decode()
    assert out.returncode == 0, (out.returncode, txt[-1000:], out.stderr.decode()[-2000:])
    kinds = {int(i): int(k) for i, k in re.findall(r"^kind (\d+) (\d+)$", txt, re.M)}
    if kinds != {0: 1, 299: 1}:
        pytest.skip("no host-visible device memory on this box: %s" % gpu.sb_host_visible_reason().decode())
    free = {k: int(v) for k, v in re.findall(r"^free (before|held|after) (\d+)$", txt, re.M)}
    print("free device memory: %r" % free)
    assert "readback mismatches 0" in txt
    assert free["after"] == free["before"], free
    assert free["before"] - free["held"] >= 300 * (64 << 10), free
