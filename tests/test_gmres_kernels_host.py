"""Pins tests/gmres_kernels_ref.py -- the GMRES loop's kernels restated launch by launch, the yardstick of
tests/test_gpu_gmres_kernels_alone.py -- on the CPU: the restated launches chained in the order sb_gmres_start / gm_step /
sb_gmres_finish enqueue them reproduce k, both histories, x and the cycle count of gmres_ref.solve bit for bit, for the fused
list and for the op list.  Every step is enqueued whether or not the loop has exited, as on the device."""
import numpy as np
import pytest

from oracle import pyoracle as po

import gmres_kernels_ref as gk
import gmres_ref

CASES = ["cd_10_11_13_m30", "cd16_m10", "cd16_m1"]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def chain(op, b, m, itermax, eps, fused):
    """the launches of one sb_gmres_solve"""
    n = len(b)
    nG = gk.groups(n)
    cap = itermax + 2
    S = gk.Block(itermax=itermax, eps=eps, hist_cap=cap)
    D = gk.Dense(m)
    st = dict(S=S, D=D, res=np.full(cap, -1.0), rr=np.full(cap, -1.0), x=np.zeros(n), r=np.zeros(n), w=np.zeros(n),
              V=[np.zeros(n) for _ in range(m + 1)], partials=np.zeros(4 * nG), launches=0)

    def true_residual(stopped):
        if stopped:
            return
        Ap = op.spmv(st["x"])
        st["r"] = po.waxpby(1.0, b, -1.0, Ap)  # (dot_spans_k<2> and the op list's waxpby: the same bits)
        st["partials"] = gk.level0(st["r"], st["r"])

    def close(mode, nvec, use_stop):
        S = st["S"]
        stopped = use_stop and S.stop
        st["D"] = gk.backsolve(S, st["D"], nvec, use_stop)
        if fused:
            st["x"], _, _ = gk.multiadd(-1, 0.0, st["V"][:nvec], st["D"].y[:nvec], st["x"], None, stopped)
        elif not stopped:
            for i in range(nvec):  # waxpby_sdev_k: x = x + y[i] * V[i]
                st["x"] = po.waxpby(1.0, st["x"], float(st["D"].y[i]), st["V"][i])
        true_residual(stopped)
        st["S"], st["res"], st["rr"] = gk.rr(mode, S, st["partials"], nG, 0, st["res"], st["rr"], use_stop)

    def step(j):
        nvec = j + 1
        V = st["V"]
        if j == 0:
            out, g0, _, _ = gk.scale(-1, 0.0, st["r"], st["S"].normr, None, st["S"].stop)
            if out is not None:
                V[0] = out
                st["D"] = st["D"].copy()
                st["D"].g[0] = g0
        stopped = st["S"].stop
        if not stopped:
            st["w"] = op.spmv(V[j])
        D = st["D"].copy()
        if fused:
            l1 = gk.multidot(V[:nvec], st["w"], stopped)
            f = gk.finish_dots(nG, l1, nG, 1, nvec, None, stopped)
            if f:
                D.h1[:nvec], D.nh1[:nvec] = f[0], f[1]
            st["w"], l1n = gk.project(2, V[:nvec], D.h1[:nvec], st["w"], stopped)
            l1 = l1 if l1n is None else l1n
            f = gk.finish_dots(nG, l1, nG, 1, nvec, D.h1, stopped)
            if f:
                D.h2[:nvec], D.nh2[:nvec], D.hcol[:nvec] = f
            st["w"], l1n = gk.project(1, V[:nvec], D.h2[:nvec], st["w"], stopped)
            l1 = l1 if l1n is None else l1n
            st["S"], st["D"], st["res"], v, _, _ = gk.step(True, -1, 0.0, st["S"], D, j, l1, nG, 1, st["w"], None, st["res"])
            if v is not None:
                V[j + 1] = v
        else:
            for h, nh, second in ((D.h1, D.nh1, False), (D.h2, D.nh2, True)):
                for i in range(nvec):
                    if not stopped:
                        st["partials"] = gk.level0(V[i], st["w"])
                    f = gk.finish_dots(nG, st["partials"], 0, 0, 1, D.h1[i:] if second else None, stopped)
                    if f:
                        h[i], nh[i] = f[0][0], f[1][0]
                        if second:
                            D.hcol[i] = f[2][0]
                if not stopped:
                    for i in range(nvec):  # waxpby_sdev_k: w = w + (-h[i]) * V[i]
                        st["w"] = po.waxpby(1.0, st["w"], float(nh[i]), V[i])
            if not stopped:
                st["partials"] = gk.level0(st["w"], st["w"])
            st["S"], st["D"], st["res"], _, _, _ = gk.step(False, -1, 0.0, st["S"], D, j, st["partials"], nG, 0, None, None, st["res"])
            out, _, _, _ = gk.scale(-1, 0.0, st["w"], st["S"].hn, None, st["S"].stop)
            if out is not None:
                V[j + 1] = out
        if j + 1 == m:
            close(1, m, 1)

    true_residual(0)
    st["S"], st["res"], st["rr"] = gk.rr(0, st["S"], st["partials"], nG, 0, st["res"], st["rr"], 0)
    pos = 0
    for _ in range(max(itermax - 1, 0)):
        step(pos)
        pos = 0 if pos + 1 == m else pos + 1
    k = st["S"].k
    if st["S"].j > 0:
        close(2, st["S"].j, 0)
    S = st["S"]
    return dict(k=k, res=st["res"][:S.n_res], rr=st["rr"][:S.n_rr], x=st["x"], cycles=S.cycles, S=S,
                tails=(st["res"][S.n_res:], st["rr"][S.n_rr:]))


@pytest.fixture(scope="module")
def problems(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gmres_kernels_host")
    out = {}
    for name in CASES:
        op, b, m, itermax, eps = gmres_ref.build_case(name, tmp)
        out[name] = (op, b, m, itermax, eps, gmres_ref.solve(op, b, m, itermax, eps))
    return out


def compare(got, want, what):
    assert got["k"] == want["k"], (what, got["k"], want["k"])
    assert same_bits(got["res"], want["res"]), (what, "res_hist")
    assert same_bits(got["rr"], want["rr"]), (what, "rr_hist")
    assert same_bits(got["x"], want["x"]), (what, "x")
    assert got["cycles"] == len(want["closes"]), (what, "cycles", got["cycles"], len(want["closes"]))
    assert all(np.all(t == -1.0) for t in got["tails"]), (what, "a history entry behind its counter was written")


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "oplist"])
@pytest.mark.parametrize("name", CASES)
def test_chained_launches_equal_the_restatement_of_the_solve(problems, name, fused):
    op, b, m, itermax, eps, want = problems[name]
    got = chain(op, b, m, itermax, eps, fused)
    compare(got, want, (name, fused))
    assert got["S"].stop == 1
    if name == "cd_10_11_13_m30":  # 1 430 rows, off the 256 grid; a full cycle, then one the exit leaves open for sb_gmres_finish
        assert len(b) == 1430 and want["k"] < itermax and got["cycles"] == 2 and (want["k"] - 1) % m != 0
    elif name == "cd16_m10":
        assert got["cycles"] > 3
    else:
        assert got["cycles"] == want["k"] - 1


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "oplist"])
@pytest.mark.parametrize("itermax", [0, 1, 2, 11, 12])
def test_chained_launches_at_the_iteration_cap(problems, itermax, fused):
    """itermax 0 / 1: no step; 2: one step; 11 / 12 with m = 10: the cap falls on a full cycle's close and one step behind it"""
    op, b, m, _, eps, _ = problems["cd16_m10"]
    want = gmres_ref.solve(op, b, m, itermax, eps)
    got = chain(op, b, m, itermax, eps, fused)
    compare(got, want, (itermax, fused))
    assert got["k"] == max(itermax, 1)


def test_the_dense_state_packs_in_the_handles_order():
    m = 3
    D = gk.Dense(m, np.arange(m * (m + 1) + 3 * m + 6 * (m + 1), dtype=np.float64))
    assert D.h(2, 1) == 1 * (m + 1) + 2 and D.cs[0] == 12 and D.sn[0] == 15 and D.y[0] == 18 and D.g[0] == 21 and D.h1[0] == 25
    assert D.h2[0] == 29 and D.nh1[0] == 33 and D.nh2[0] == 37 and D.hcol[0] == 41 and D.hcol[-1] == 44
    assert np.array_equal(D.pack(), np.arange(45.0))
    E = D.copy()
    E.y[0] = -1.0
    assert D.y[0] == 18


def test_scalar_kernels_leave_what_they_must():
    """the guards the GPU scenarios rest on, on the restatement itself"""
    h = np.array([7.0, 8.0])
    q = np.array([4.0])
    S = gk.Block(k=5, itermax=9, eps=1.0, n_rr=2, n_res=2, hist_cap=2, cycles=1, j=3, normr=0.5)
    o, res, rr = gk.rr(2, S, q, 1, 1, h, h, 0)
    assert res is h and rr is h and (o.rr, o.n_rr, o.cycles, o.j, o.normr, o.stop) == (4.0, 3, 2, 0, 0.5, 0)
    o, res, rr = gk.rr(1, S, q, 1, 1, h, h, 1)
    assert (o.normr, o.stop, o.k) == (2.0, 0, 5)
    o, _, _ = gk.rr(1, S.copy(eps=2.0), q, 1, 1, h, h, 1)
    assert o.stop == 1  # normr == eps ends the loop
    o, _, _ = gk.rr(1, S.copy(k=9), q, 1, 1, h, h, 1)
    assert o.stop == 1
    o, res, rr = gk.rr(1, S.copy(stop=1), q, 1, 1, h, h, 1)
    assert o.i().tolist() == S.copy(stop=1).i().tolist() and o.rr == 0.0
    o, res, rr = gk.rr(0, gk.Block(itermax=1, hist_cap=0, eps=0.0), q, 1, 1, h, h, 0)
    assert res is h and rr is h and (o.stop, o.k, o.n_res, o.n_rr, o.normr) == (1, 1, 1, 1, 2.0)
    # the scalar step: hn = 0 gives d = |hjj|, s = 0; a block that arrives stopped changes nothing
    D = gk.Dense(2)
    D.hcol[:] = [-3.0, 0.0, 0.0]
    D.g[0] = 2.0
    S = gk.Block(k=1, itermax=9, eps=0.0, hist_cap=4)
    o, E, res, v, d, z = gk.step(True, -1, 0.0, S, D, 0, np.array([0.0]), 1, 1, np.array([1.0]), None, np.zeros(4))
    assert (E.H[0], E.cs[0], E.sn[0], E.g[0], o.normr, o.stop, o.k, o.j, o.steps) == (3.0, -1.0, 0.0, -2.0, 0.0, 1, 2, 1, 1)
    assert str(E.g[1]) == "-0.0" and res[1] == 0.0
    o2, E2, res2, v, d, z = gk.step(True, -1, 0.0, o, E, 1, np.array([1.0]), 1, 1, np.array([1.0]), None, res)
    assert o2 is o and E2 is E and res2 is res and v is None


ENTRIES = {"sb_gmres_multidot_native": 7, "sb_gmres_finish_dots_native": 10, "sb_gmres_project_native": 9, "sb_gmres_multiadd_native": 12,
           "sb_gmres_scale_native": 11, "sb_gmres_rr_native": 9, "sb_gmres_step_native": 18, "sb_gmres_backsolve_native": 6,
           "sb_gmres_scale_launch": 2, "sb_gmres_step_launch": 2, "sb_gmres_group_launch": 2}


def test_entries_declared_exported_and_listed():
    """the blocking entries and launch queries: in include/sbhip.h, exported by the library, listed in capi with a prototype of
    as many parameters as the declaration; the control block is 4 doubles and 9 ints as the header says"""
    import ctypes
    import os
    import re
    from sparsebench_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sbhip.h")).read()
    L = capi.load()
    for name, count in ENTRIES.items():
        decl = re.search(r"\b(int|void) %s\s*\(([^)]*)\)" % name, header)
        assert decl, name
        assert name in capi.SYMBOLS and hasattr(L, name)
        fn = getattr(L, name)
        assert len(decl.group(2).split(",")) == count == len(fn.argtypes), (name, decl.group(2))
        assert fn.restype is (ctypes.c_int if decl.group(1) == "int" else None)
    flat = " ".join(header.replace(" *", " ").split())
    assert "blk_d[4] = {%s}" % ", ".join(gk.FIELDS_D) in flat
    assert "blk_i[9] = {%s}" % ", ".join(gk.FIELDS_I) in flat
    assert L.sb_is_initialized() == 0  # loading touched no device
