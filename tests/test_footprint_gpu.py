"""Write footprint and per-rank buffer alignment of every collective and of
the local fold (tests/footprint.py, tests/spmd/footprint_worker.py): each
buffer sits between a 4 KiB and a 64 KiB guard at a byte offset of its rank's
own, and every call is checked for its result (bit-exact against
oracle/mpich_model.py / tests/redscat_model.py), untouched guards and pad, an
unchanged sendbuf, and wholly unchanged buffers where the call may only read
(a Reduce non-root's non-null recvbuf, Exscan's rank 0, Bcast's root).

One worker launch runs the whole table of its world size; all ranks share
cuda:0 and MPIGX_MAX_BLOCKS=16 keeps every rank's grid co-resident (see
test_collectives_gpu.py).
"""
import ctypes
import json
import os

import numpy as np
import pytest

import footprint as F
from oracle import mpich_model as M
from spmd_launch import ROOT, launch
from test_collectives_gpu import ENV

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "spmd", "footprint_worker.py")


def _run(n, table, cs, **extra):
    ncases = len(cs)
    env = dict(ENV, FP_TABLE=table, **extra)
    rcs, outs = launch(WORKER, n, timeout=240, extra_env=env)
    msg = "\n".join(f"--- rank {r} rc={rc}\n{o[-3000:]}" for r, (rc, o) in enumerate(zip(rcs, outs)))
    summ = [json.loads(l) for o in outs for l in o.splitlines() if l.startswith("{") and '"checks"' in l]
    print(json.dumps([{k: s[k] for k in ("rank", "cases", "checks", "nfail", "zc_exchanges", "zc_hits")} for s in summ]))
    assert all(rc == 0 for rc in rcs), msg
    # one check per call (its return code) and one per buffer verified: at least the recvbuf
    assert len(summ) == n and all(x["nfail"] == 0 and x["checks"] >= 2 * ncases for x in summ), summ
    # the zero-copy cases ran zero-copy: ZC_REQUIRE turns a fall-back into an error, and every such call
    # exchanged its buffers or hit the optimistic view of an earlier exchange
    if F.zc_calls(cs):
        assert all(x["zc_exchanges"] > 0 and x["zc_exchanges"] + x["zc_hits"] >= F.zc_calls(cs) for x in summ), summ
    return summ


def _main(n, **extra):
    _run(n, "main", F.cases(n), **extra)


@pytest.mark.parametrize("n", [3, 8])
def test_collectives_footprint(n):
    """(~8 s) The whole table (every Allreduce algorithm, Reduce, Bcast, Allgather, Alltoall, Scan, Exscan,
    Reduce_scatter_block and Reduce_scatter; staged and zero-copy; in place and out of place) at n = 3
    (pre-step, rem 1, NMAX 4) and n = 8 (full tree, NMAX 8), every rank at its own buffer alignment."""
    _main(n)


def test_collectives_footprint_xdev():
    """(~4 s) The table at n = 5 under MPIGX_PEER_MEM=xdev (the one-rank-per-GPU signalling)."""
    _main(5, MPIGX_PEER_MEM="xdev")


def test_small_arena_round_boundaries():
    """(~4 s) n = 3 with the arena at its floor (4096 B): Allreduce, Reduce, Bcast and Reduce_scatter staged in
    at least four rounds each, so every round boundary is a footprint edge."""
    cs = F.small_arena_cases(3)
    assert all(F.rounds(c, 3) >= 3 for c in cs)
    _run(3, "small", cs, MPIGX_STAGING_BYTES=str(F.SMALL_STAGE))


@pytest.mark.slow
@pytest.mark.parametrize("n", [2, 6, 7])
def test_collectives_footprint_more_sizes(n):
    """(~13 s) The table at n = 2 (NMAX 2), n = 6 (rem 2) and n = 7 (rem 3, every partition cut in seven)."""
    _main(n)


@pytest.mark.slow
def test_collectives_footprint_stream_ordered():
    """(~4 s) The table at n = 3 stream-ordered: set_blocking(0), mpigx_comm_synchronize before the read-back."""
    _main(3, FP_STREAM="1")


# ---------------------------------------------------------------------------
# the local fold, in process
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import mpigx
    import torch
    assert torch.cuda.is_available()
    return mpigx.lib()


def _up(g):
    import torch
    t = torch.empty(g.image.size, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % F.ALIGN == 0
    t.copy_(torch.from_numpy(g.image))
    return t


def _fold(L, ins, dt, op, order, in_offs, out_off, salt, check_inputs):
    """One mpigx_reduce_local_multi call on guarded buffers; returns the findings."""
    import torch
    npdt = np.dtype(M.DTYPES[dt][1])
    exp = M.fold_linear(ins, dt, op) if order else M.allreduce(ins, dt, op)[0]
    kw = {"npdt": npdt, "bf16": dt == "BFLOAT16"}
    gin = [F.Guarded(x, o, k, salt + k, readonly=True, **kw) for k, (x, o) in enumerate(zip(ins, in_offs))]
    gout = F.Guarded(None, out_off, 99, salt, nbytes=ins[0].nbytes, expect=exp, **kw)
    tin = [_up(g) for g in gin]
    tout = _up(gout)
    ptrs = (ctypes.c_void_p * len(ins))(*[t.data_ptr() + g.lo for t, g in zip(tin, gin)])
    rc = L.mpigx_reduce_local_multi(ptrs, len(ins), ctypes.c_void_p(tout.data_ptr() + gout.lo), ins[0].size,
                                    M.DTYPES[dt][0], M.OPS[op], order, None)
    assert rc == 0
    torch.cuda.synchronize()
    found = [dict(f, buf="out") for f in F.verify(gout, tout.cpu().numpy())]
    if check_inputs:
        for k, (g, t) in enumerate(zip(gin, tin)):
            found += [dict(f, buf=f"in{k}") for f in F.verify(g, t.cpu().numpy())]
    return found


def _offsets(kind, nin, dt, k, align=None):
    """Byte offsets of the inputs and the output: the per-rank table, all
    aligned but one input, only the output misaligned."""
    es = F.esize(dt)
    a = align or F.comp_align(dt)
    mis = a
    if kind == 0:
        return [F.send_off(i, es, a) for i in range(nin)], F.recv_off(2 + k % 6, es, a)
    if kind == 1:
        return [mis if i == k % nin else 0 for i in range(nin)], 0
    return [0] * nin, mis


def test_local_fold_footprint(L):
    """(~2 s) mpigx_reduce_local_multi with 2, 5 and 8 inputs at MPIGX_LOCAL_U 1 / 2 / 4: every input at its
    own byte offset (the per-rank table, all aligned but one, only the output misaligned), the output
    guarded on both sides, the inputs unchanged; the table's counts plus one just past a U * kThreads
    vector block (the write-through span path with a partial last span).  mpigx_reduce_local: the inoutbuf's
    guards and the `in` buffer unchanged."""
    from gen_inputs import make
    bad, k = [], 0
    try:
        for u in (1, 2, 4):
            os.environ["MPIGX_LOCAL_U"] = str(u)
            for nin in (2, 5, 8):
                for dt, ops in F.DTYPE_OPS:
                    w = max(1, 16 // F.esize(dt))
                    for count in F.counts_for(dt, 8) + (u * 256 * w + 3,):
                        op = ops[k % len(ops)]
                        ins = make(dt, op, nin, count, 300 + k, edge=k % 2 == 0)
                        in_offs, out_off = _offsets(k % 3, nin, dt, k)
                        for f in _fold(L, ins, dt, op, (k // 3) % 2, in_offs, out_off, 11 * k, k % 3 == 0):
                            bad.append(dict(f, u=u, nin=nin, dtype=dt, op=op, count=count, offs=(in_offs, out_off)))
                        k += 1
    finally:
        os.environ.pop("MPIGX_LOCAL_U", None)
    assert not bad, bad[:6]
    assert k == 3 * 3 * len(F.DTYPE_OPS) * 7
    # control: the harness sees device stores.  A fold of 5 more elements than the output's payload holds
    # (inside the allocation: the post-guard is 64 KiB) must be reported in the first 20 post-guard bytes, and nowhere else.
    ins = make("FLOAT", "SUM", 3, 1001 + 5, 1)
    exp = M.allreduce(ins, "FLOAT", "SUM")[0][:1001]
    g = F.Guarded(None, 4, 99, 3, nbytes=1001 * 4, expect=exp, npdt=np.dtype(np.float32))
    tin = [_up(F.Guarded(x, 0, i, 5, readonly=True)) for i, x in enumerate(ins)]
    t = _up(g)
    ptrs = (ctypes.c_void_p * 3)(*[ti.data_ptr() + F.PRE for ti in tin])
    assert L.mpigx_reduce_local_multi(ptrs, 3, ctypes.c_void_p(t.data_ptr() + g.lo), 1006, M.DTYPES["FLOAT"][0],
                                      M.OPS["SUM"], 0, None) == 0
    import torch
    torch.cuda.synchronize()
    found = F.verify(g, t.cpu().numpy())
    assert [f["kind"] for f in found] == ["post"] and g.hi <= found[0]["offset"] < g.hi + 20, found
    # MPI_Reduce_local: inout = op(inout, in)
    import torch
    for j, (dt, ops) in enumerate(F.DTYPE_OPS):
        es, a = F.esize(dt), F.comp_align(dt)
        npdt = np.dtype(M.DTYPES[dt][1])
        for count in F.counts_for(dt, 2):
            op = ops[(j + count) % len(ops)]
            x, y = make(dt, op, 2, count, 700 + j + count, edge=True)
            kw = {"npdt": npdt, "bf16": dt == "BFLOAT16"}
            gi = F.Guarded(x, F.send_off(1 + count % 7, es, a), 0, 5 * j, readonly=True, **kw)
            go = F.Guarded(y, F.recv_off(2 + count % 6, es, a), 1, 5 * j + 1, expect=M.reduce_local(x, y, dt, op), **kw)
            ti, to = _up(gi), _up(go)
            rc = L.mpigx_reduce_local(ctypes.c_void_p(ti.data_ptr() + gi.lo), ctypes.c_void_p(to.data_ptr() + go.lo),
                                      count, M.DTYPES[dt][0], M.OPS[op])
            assert rc == 0
            torch.cuda.synchronize()
            found = F.verify(go, to.cpu().numpy()) + F.verify(gi, ti.cpu().numpy())
            assert not found, (dt, op, count, found)


def test_component_aligned_complex():
    """(~4 s) C_DOUBLE_COMPLEX at byte offset 8 and C_FLOAT_COMPLEX at 4 / 8 / 12 (legal in MPI, what a numpy
    view gives; element-granular offsets never produce them): the local fold in process, then the staged
    two-shot and the zero-copy pull Allreduce at n = 3.  On its own, so whatever happens here does not mask
    the rest."""
    import mpigx
    from gen_inputs import make
    lib = mpigx.lib()
    bad, k = [], 0
    for dt in ("C_DOUBLE_COMPLEX", "C_FLOAT_COMPLEX"):
        for nin in (2, 5, 8):
            for count in F.counts_for(dt, 8):
                op = ("SUM", "PROD")[k % 2]
                ins = make(dt, op, nin, count, 900 + k)
                in_offs, out_off = _offsets(k % 3, nin, dt, k)
                for f in _fold(lib, ins, dt, op, (k // 3) % 2, in_offs, out_off, 13 * k, True):
                    bad.append(dict(f, nin=nin, dtype=dt, op=op, count=count, offs=(in_offs, out_off)))
                k += 1
    assert not bad, bad[:6]
    _run(3, "complex", F.complex_cases(3))
