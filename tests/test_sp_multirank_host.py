"""Single precision on several ranks, on the CPU: the numpy P-rank restatement (tests/sp_mpi_ref.py) reproduces the reference's
own SP MPI histories (tests/golden/cg_hist_sp_mpi.json) bit for bit in the seq order -- which pins MPICH's MPI_FLOAT SUM as the
pairwise tree in rank order --, the layer's float rank reduction (sb_rank_reduce_f32, what the host transport's all-reduce adds
with) is that tree, and the new entry points are exported and link from C with -DPRECISION=1."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import sp_mpi_ref
from oracle import pyoracle as po
from sparsebench_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cg_hist_sp_mpi.json")
BAND = os.path.join(ROOT, "tests", "golden", "ref", "matrix_band_klein.mtx")
LIB = os.path.join(ROOT, "sparsebench_amd", "lib")
F = np.float32


def bits(a):
    return np.asarray(a, F).view(np.uint32)


def test_golden_well_formed():
    g = json.load(open(GOLDEN))
    assert sorted(g) == ["band_klein_x2", "hpcg16_x2", "hpcg16_x4", "hpcg8_x8"]
    for name, c in g.items():
        for key in ("rr", "pAp"):
            v = np.array([float(s) for s in c[key]])
            assert np.array_equal(v.astype(F).astype(np.float64), v), (name, key)  # every value is a float
        assert len(c["rr"]) == c["k"] - 1 and len(c["pAp"]) == c["k"] - 1


@pytest.mark.parametrize("name", ["hpcg16_x2", "hpcg16_x4", "hpcg8_x8", "band_klein_x2"])
def test_restatement_seq_reproduces_reference_mpi(name):
    g = json.load(open(GOLDEN))[name]
    src = BAND if name.startswith("band") else name.split("_")[0]
    locs, plans, keep = sp_mpi_ref.locals_and_plans(po, src, g["ranks"])
    k, rr, pap, x = sp_mpi_ref.cg(locs, plans, g["itermax"], dot="seq")
    assert k == g["k"]
    assert np.array_equal(bits(rr), bits([float(v) for v in g["rr"]])), name
    assert np.array_equal(bits(pap), bits([float(v) for v in g["pAp"]])), name
    for loc in locs:
        loc.free()


def _tree(vals, op):
    return sp_mpi_ref.rank_sum(vals) if op == 1 else sp_mpi_ref.rank_max(vals)


@pytest.mark.parametrize("P", range(2, 9))
def test_rank_reduce_is_the_pairwise_float_tree(P):
    L = capi.load()  # (host code: no device needed)
    rng = np.random.default_rng(P)
    tiny = np.float32(1.4e-45)  # the smallest f32 subnormal
    cases = [
        rng.standard_normal(P).astype(F) * F(1e3),
        (rng.integers(1, 1000, P) * tiny).astype(F),                                # subnormals only
        np.array([(1e8 if i % 2 == 0 else -1e8) + i for i in range(P)], F),        # cancelling
        np.array([F(1.0)] + [F(2.0 ** -24)] * (P - 1), F),                          # order decides the rounding
        np.array([F(3.0e38)] * P, F),                                               # overflow to inf in float
    ]
    for v in cases:
        for op in (0, 1):
            got = L.sb_rank_reduce_f32(v.ctypes.data_as(C.c_void_p), P, op)
            want = _tree(list(v), op)
            assert F(got).view(np.uint32) == want.view(np.uint32), (P, op, v, got, want)
    if P == 3:  # ((1 + u) + u) with u = 2^-24 rounds to 1 twice; widened to double and rounded once it would be 1 + 2^-23
        v = np.array([1.0, 2.0 ** -24, 2.0 ** -24], F)
        assert L.sb_rank_reduce_f32(v.ctypes.data_as(C.c_void_p), 3, 1) == 1.0 != F(v.astype(np.float64).sum())


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_new_entry_points_exported():
    syms = _exports(os.path.join(LIB, "libsbhip.so"))
    for s in ("sb_halo_exchange_f32", "sb_comm_reduction_f32", "sb_rank_reduce_f32"):
        assert s in syms and s in capi.SYMBOLS, s
    host = _exports(os.path.join(LIB, "libsparsebench_host_sp.so"))
    assert {"commExchange", "commReduction"} <= host


PROBE = r"""
#include <sparsebench/sparsebench.h>
#include "sbhip.h"
#include <stdio.h>
_Static_assert(sizeof(CG_FLOAT) == 4, "PRECISION=1");
int main(int argc, char** argv)
{
  void (*ex)(sb_halo*, float*) = sb_halo_exchange_f32;
  void (*red)(float*, int) = sb_comm_reduction_f32;
  void (*cx)(Comm*, CG_UINT, CG_FLOAT*) = commExchange;
  void (*cr)(CG_FLOAT*, int) = commReduction;
  const float v[3] = { 1.0f, 2.0f, 4.0f };
  printf("%d %g\n", argc > 5 && ex && red && cx && cr, (double)sb_rank_reduce_f32(v, 3, 1));
  return 0;
}
"""


def test_c_probe_links_sp_entry_points(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Werror", "-DPRECISION=1", "-I" + inc, "-I" + inc + "/sparsebench", str(src),
                           "-o", str(exe), "-L" + LIB, "-lsparsebench_host_sp", "-lsbhip", "-Wl,-rpath," + LIB])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["0", "7"], out.stdout


def test_problem_names_of_the_multirank_cases():
    """"hpcgN" is an N^3 brick per rank, "hpcgXxYxZ" an X x Y x Z one (tests/gpu_sp_multirank_worker.py)"""
    assert sp_mpi_ref.hpcg_dims("hpcg16") == (16, 16, 16) and sp_mpi_ref.hpcg_dims("hpcg7x7x9") == (7, 7, 9)
    locs, plans, keep = sp_mpi_ref.locals_and_plans(po, "hpcg7x7x9", 3)
    assert [g.nr for g in locs] == [441, 441, 441] and [pl["externalCount"] for pl in plans] == [49, 98, 49]
    for g in locs:
        g.free()
