"""fp32 restatement of single-precision CG on P ranks, for the tests only (numpy; the product never imports it).

Built on tests/sp_ref.py (every operation a float32 operation in the reference's order) and on the oracle's partition
(oracle/pyoracle.py: GMatrix.generate / from_mtx, Plans): each rank's local CRS matrix with its halo columns behind its nr
rows, the halo delivered from the plans (src/comm.c:627-649), every dot a per-rank sum -- tree order over the rank's rows in
the device's row order, or seq over its rows in original order -- followed by the rank sum of MPI_Allreduce(MPI_FLOAT, SUM):
pairwise in rank order, ((v0 + v1) + (v2 + v3)) + ..., in float32 (what MPICH does, and what every data plane of the layer
does: include/sbhip.h sb_comm_reduction_f32).
"""
import numpy as np

import sp_ref

F = np.float32


def rank_sum(values):
    """pairwise float32 tree in rank order; an odd tail moves up unchanged"""
    v = [F(x) for x in values]
    with np.errstate(over="ignore", invalid="ignore"):
        while len(v) > 1:
            nxt = [F(v[i] + v[i + 1]) for i in range(0, len(v) - 1, 2)]
            if len(v) & 1:
                nxt.append(v[-1])
            v = nxt
    return F(v[0])


def rank_max(values):
    m = F(values[0])
    for x in values[1:]:
        if F(x) > m:
            m = F(x)
    return m


def hpcg_dims(name):
    """"hpcgN" -> (N, N, N), "hpcgXxYxZ" -> (X, Y, Z)"""
    d = [int(v) for v in name[4:].split("x")]
    assert len(d) in (1, 3), name
    return tuple(d * 3) if len(d) == 1 else tuple(d)


def locals_and_plans(po, name, size):
    """the P local matrices (oracle-owned) and their halo plans: name = "hpcgN", "hpcgXxYxZ" or a .mtx path"""
    if name.startswith("hpcg"):
        nx, ny, nz = hpcg_dims(name)
        locs = [po.GMatrix.generate(nx, ny, nz, r, size) for r in range(size)]
    else:
        locs = [po.GMatrix.from_mtx(name, r, size) for r in range(size)]
    plans = po.Plans(locs)
    return locs, [plans.plan(r) for r in range(size)], plans


def halo_fill(ps, plans):
    """p with its externals behind the nr rows on every rank: rank s's block for r, elementsToSend in order, lands at r's
    rdispl for s"""
    out = []
    for r, pl in enumerate(plans):
        ext = np.zeros(pl["externalCount"], F)
        for j in range(pl["indegree"]):
            s = int(pl["sources"][j])
            ps_ = plans[s]
            i = list(ps_["destinations"]).index(r)
            idx = ps_["elementsToSend"][ps_["sdispls"][i]:ps_["sdispls"][i] + ps_["sendCounts"][i]]
            ext[pl["rdispls"][j]:pl["rdispls"][j] + pl["recvCounts"][j]] = ps[s][idx]
        out.append(np.concatenate([ps[r], ext]).astype(F))
    return out


def cg(locs, plans, itermax, dot="tree", orders=None, eps=0.0):
    """solveCG of the SP build on len(locs) ranks.  orders[r]: rank r's device row order (newToOld of Sell-C-sigma, sigma > 1)
    for the tree dot, None = original order.  Returns (k, rr, pAp, [x per rank])."""
    P = len(locs)
    mats = [(np.asarray(g.rowPtr, np.int64), np.asarray(g.col, np.int64), g.val.astype(F)) for g in locs]
    bs = [g.rhs().astype(F) for g in locs]
    orders = orders or [None] * P

    def spmv(ps):
        full = halo_fill(ps, plans)
        return [sp_ref.spmv_crs(m[0], m[1], m[2], full[r]) for r, m in enumerate(mats)]

    def ddot(a, b):
        vals = []
        for r in range(P):
            if dot == "seq":
                vals.append(sp_ref.dot_seq(a[r], b[r]))
            else:
                o = orders[r]
                vals.append(sp_ref.dot_tree(a[r], b[r]) if o is None else sp_ref.dot_tree(a[r][o], b[r][o]))
        return rank_sum(vals)

    wax = lambda al, x, be, y: [sp_ref.waxpby(al, x[r], be, y[r]) for r in range(P)]
    x = [np.zeros(len(b), F) for b in bs]
    p = wax(1.0, x, 0.0, x)
    Ap = spmv(p)
    r = wax(1.0, bs, -1.0, Ap)
    rtrans = ddot(r, r)
    rr, pap = [rtrans], []
    fails = sp_ref.normr_fails(rtrans, eps)
    k = 1
    with np.errstate(all="ignore"):
        while k < itermax and not fails:
            if k == 1:
                p = wax(1.0, r, 0.0, r)
            else:
                old = rtrans
                rtrans = ddot(r, r)
                rr.append(rtrans)
                beta = F(rtrans / old)
                p = wax(1.0, r, beta, p)
            fails = sp_ref.normr_fails(rtrans, eps)
            Ap = spmv(p)
            t = ddot(p, Ap)
            pap.append(t)
            alpha = F(rtrans / t)
            x = wax(1.0, x, alpha, p)
            r = wax(1.0, r, -alpha, Ap)
            k += 1
    return k, np.array(rr, F), np.array(pap, F), x
