"""Host-mediated transport over torch.distributed (gloo) for the multi-rank device path.

The production data plane is RCCL inside libsbhip.so (sb_comm_init).  A launcher without
RCCL -- or several ranks sharing one GPU, which RCCL refuses -- supplies two callbacks instead
(include/sbhip.h: sb_transport, sb_comm_init_transport) and an sbh_exchange for the setup
traffic of commPartition.  This module is that launcher-side glue for torch.distributed:
device buffers are staged through the host, gloo moves them.  Used by
tests/gpu_multirank_worker.py and by `bench.py --transport host` (rehearsal of the N-rank
bench flow on one GPU); correct, not fast.
"""
import ctypes as C
import os

import numpy as np

from . import capi, hostapi

vp = C.c_void_p


def attach(L, H, dist, rank, size, allgather_bytes=True):
    """Install the setup exchange (H.commSetExchange) and the run-time transport
    (L.sb_comm_init_transport).  Returns the ctypes objects that must stay alive.

    H: the host library whose commPartition runs on these ranks -- hostapi.host("single") for single precision, whose
    float all-reduce (sb_comm_reduction_f32) gathers the ranks' float32 values through allgather_bytes and adds them
    pairwise in rank order inside the layer.  allgather_bytes=False leaves that optional callback out, as a launcher
    without one would (the peer-mapped set-up, which needs it for the halo handles, is then skipped as well)."""
    import torch

    def allgather(ctx, mine, cnt, out):
        t = torch.tensor([mine[i] for i in range(cnt)], dtype=torch.int32)
        outs = [torch.zeros(cnt, dtype=torch.int32) for _ in range(size)]
        dist.all_gather(outs, t)
        for i, v in enumerate(torch.cat(outs).tolist()):
            out[i] = v

    def alltoallv(ctx, sbuf, scnt, sdsp, rbuf, rcnt, rdsp):
        reqs, recv = [], {}
        for r in range(size):
            if r == rank:
                continue
            if scnt[r]:
                reqs.append(dist.isend(torch.tensor([sbuf[sdsp[r] + i] for i in range(scnt[r])], dtype=torch.int32), r))
            if rcnt[r]:
                recv[r] = torch.zeros(rcnt[r], dtype=torch.int32)
                reqs.append(dist.irecv(recv[r], r))
        for q in reqs:
            q.wait()
        for r, t in recv.items():
            for i, v in enumerate(t.tolist()):
                rbuf[rdsp[r] + i] = v

    def d2h(ptr, count):
        a = np.empty(count, dtype=np.float64)
        if count:
            L.sb_d2h(a.ctypes.data_as(vp), ptr, count * 8)
        return a

    def allreduce(ctx, v_dev, op):
        mine = torch.from_numpy(d2h(v_dev, 1))
        outs = [torch.zeros(1, dtype=torch.float64) for _ in range(size)]
        dist.all_gather(outs, mine)
        vals = [float(t[0]) for t in outs]
        if op == 0:
            res = max(vals)
        else:  # pairwise tree == recursive doubling of the MPI reference run
            while len(vals) > 1:
                nxt = [vals[i] + vals[i + 1] for i in range(0, len(vals) - 1, 2)]
                if len(vals) & 1:
                    nxt.append(vals[-1])
                vals = nxt
            res = vals[0]
        out = np.array([res])
        L.sb_h2d(v_dev, out.ctypes.data_as(vp), 8)

    def exchange(ctx, send_dev, outdeg, dests, scnt, sdsp, recv_dev, indeg, srcs, rcnt, rdsp):
        total = sum(scnt[i] for i in range(outdeg))
        sbuf = d2h(send_dev, total)
        # TEST HOOK (bench.py's degraded completion the other way round, tests/test_gpu_bench.py): rank r's staged send / recv swaps
        # its first two values -- wrong on the communicator's plane ONLY (the peer-mapped push does not come through here)
        if os.environ.get("SB_TEST_CORRUPT_HOST_EXCHANGE") == str(rank) and total >= 2:
            sbuf = sbuf.copy()
            sbuf[0], sbuf[1] = sbuf[1], sbuf[0]
        reqs, bufs = [], []
        for i in range(outdeg):
            reqs.append(dist.isend(torch.from_numpy(sbuf[sdsp[i]:sdsp[i] + scnt[i]].copy()), dests[i]))
        for j in range(indeg):
            t = torch.zeros(rcnt[j], dtype=torch.float64)
            bufs.append((rdsp[j], t))
            reqs.append(dist.irecv(t, srcs[j]))
        for q in reqs:
            q.wait()
        for off, t in bufs:
            a = t.numpy()
            L.sb_h2d(recv_dev + off * 8, a.ctypes.data_as(vp), len(a) * 8)

    cb1, cb2 = hostapi.ALLGATHER_FN(allgather), hostapi.ALLTOALLV_FN(alltoallv)
    xchg = hostapi.ExchangeS(None, cb1, cb2)
    H.commSetExchange(C.byref(xchg))
    def allgather_bytes_cb(ctx, mine, nbytes, out):
        t = torch.tensor(list(C.string_at(mine, nbytes)), dtype=torch.uint8)
        outs = [torch.zeros(nbytes, dtype=torch.uint8) for _ in range(size)]
        dist.all_gather(outs, t)
        C.memmove(out, bytes(torch.cat(outs).tolist()), nbytes * size)

    cb3, cb4, cb5 = capi.ALLREDUCE_FN(allreduce), capi.EXCHANGE_FN(exchange), capi.ALLGATHER_BYTES_FN(allgather_bytes_cb)
    tr = capi.TransportS(None, cb3, cb4, cb5) if allgather_bytes else capi.TransportS(None, cb3, cb4)  # (unset field: NULL)
    L.sb_comm_init_transport(rank, size, C.byref(tr))
    if not allgather_bytes:
        return (cb1, cb2, xchg, cb3, cb4, tr)
    # in-kernel all-reduce over peer-mapped memory (include/sbhip.h): gather the IPC handles, open, self-test
    mine = (C.c_ubyte * 64)()
    have = L.sb_comm_p2p_handle(mine)
    t = torch.tensor(list(mine) if have else [0] * 64, dtype=torch.uint8)
    outs = [torch.zeros(64, dtype=torch.uint8) for _ in range(size)]
    dist.all_gather(outs, t)
    allh = (C.c_ubyte * (64 * size))(*torch.cat(outs).tolist())
    L.sb_comm_p2p_open(allh if have else None)
    return (cb1, cb2, xchg, cb3, cb4, cb5, tr)
