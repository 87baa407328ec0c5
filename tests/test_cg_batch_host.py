"""Pins tests/cg_batch_ref.py -- solveCG restated for an arbitrary right-hand side, the yardstick of the batched solver's
columns -- to the oracle's own CG in the tree dot order and to the committed tree-order golden, bit for bit, on the CPU."""
import numpy as np
import pytest

from oracle import pyoracle as po

import cg_batch_ref as ref
from conftest import load_json

CASES = [("crs16", (16, 16, 16), "crs", 1), ("scs16_sigma1", (16, 16, 16), "scs", 1), ("scs32_sigma256", (32, 32, 32), "scs", 256),
         ("crs_10_11_13", (10, 11, 13), "crs", 1), ("scs_10_11_13_sigma256", (10, 11, 13), "scs", 256)]


@pytest.mark.parametrize("name,dims,fmt,sigma", CASES)
def test_restatement_equals_the_oracle_cg_in_tree_order(name, dims, fmt, sigma):
    g = po.GMatrix.generate(*dims)
    want = po.cg(g, fmt=fmt, Cc=64, sigma=sigma, itermax=60, eps=0.0, dot="tree", want_x=True)
    got = ref.solve(ref.operator(g, fmt, 64, sigma), g.rhs(), 60, 0.0)
    assert got["k"] == want["k"]
    assert ref.same_bits(got["rr"], want["rr"]) and ref.same_bits(got["pAp"], want["pAp"])
    assert ref.same_bits(got["x"], want["x"][0])
    g.free()


def test_restatement_stops_where_the_oracle_stops_with_eps():
    g = po.GMatrix.generate(16, 16, 16)
    want = po.cg(g, fmt="scs", Cc=64, sigma=1, itermax=150, eps=1e-6, dot="tree", want_x=True)
    got = ref.solve(ref.operator(g, "scs", 64, 1), g.rhs(), 150, 1e-6)
    assert 1 < want["k"] < 150 and got["k"] == want["k"]
    assert ref.same_bits(got["rr"], want["rr"]) and ref.same_bits(got["pAp"], want["pAp"]) and ref.same_bits(got["x"], want["x"][0])
    g.free()


def test_restatement_equals_the_committed_tree_golden():
    e = load_json("cg_hist_tree.json")["hpcg32_x1_scs_C64_sigma256"]
    g = po.GMatrix.generate(e["n"], e["n"], e["n"])
    got = ref.solve(ref.operator(g, "scs", e["C"], e["sigma"]), g.rhs(), e["itermax"], 0.0)
    assert got["k"] == e["k"]
    assert ref.same_bits(got["rr"], np.array([float(v) for v in e["rr"]]))
    assert ref.same_bits(got["pAp"], np.array([float(v) for v in e["pAp"]]))
    g.free()


def test_rhs_rule():
    b0 = np.arange(12, dtype=np.float64)
    B = ref.batch_rhs(b0, 4, start_row=3)
    assert B.shape == (4, 12) and np.array_equal(B[0], b0)
    for c in range(4):
        for i in range(12):
            assert B[c, i] == b0[i] + c * (((3 + i) % 5) - 2)
    from sparsebench_amd import hostapi
    assert np.array_equal(hostapi.batch_rhs(b0, 4, 3), B)
