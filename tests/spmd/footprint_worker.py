"""SPMD worker of tests/test_footprint_gpu.py (one process per rank): runs the
case table of tests/footprint.py for this world size and checks, per call,
where bytes landed: the result bit for bit against the models, both guards
and the pad of the recvbuf, the sendbuf unchanged, and every buffer the call
may only read (a Reduce non-root's non-null recvbuf, Exscan's rank 0, Bcast's
root) wholly unchanged.  Every rank places its buffers at its own byte
offsets (footprint.send_off / recv_off), so the zero-copy kernels see peers'
pointers of mixed alignment.

FP_TABLE picks the table: main (footprint.cases), small (small_arena_cases:
the launcher passes MPIGX_STAGING_BYTES = footprint.SMALL_STAGE), complex
(complex_cases: component-aligned complex buffers).  FP_STREAM=1 runs the
calls stream-ordered (set_blocking(0), mpigx_comm_synchronize before the
read-back).  Paths are forced through MPI.set_knob; MAX_BLOCKS comes from the
launcher, BYTES_PER_BLOCK is lowered to its minimum so a few hundred bytes
are already cut into several chunks and slices.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "mpi.jl_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import footprint as F  # noqa: E402
import mpigx as MPI  # noqa: E402
from oracle import mpich_model as M  # noqa: E402

IN_PLACE = ctypes.c_void_p(-1 & ((1 << 64) - 1))
TABLE = os.environ.get("FP_TABLE", "main")
STREAM = os.environ.get("FP_STREAM") == "1"

comm = MPI.Init()
L = MPI.lib()
r, n, cv = MPI.Comm_rank(comm), MPI.Comm_size(comm), comm.val
FAIL, RAN = [], [0]
ZC_MIN0 = MPI.get_knob(comm, "ZC_MIN")
CUR = {}


def knob(name, value):
    if CUR.get(name) != value:
        if name == "LINEAR":
            MPI.set_reduce_order(comm, 1 if value else 0)
        else:
            MPI.set_knob(comm, name, value)
        CUR[name] = value


def apply_knobs(kn):
    zc = kn.get("ZC", 0)
    knob("ZC_MIN", 1 if zc else ZC_MIN0)
    knob("ZC_REQUIRE", 1 if zc else 0)
    knob("ALGO", kn.get("ALGO", "auto"))
    knob("BCAST", kn.get("BCAST", "auto"))
    knob("RING_CHANNELS", kn.get("RING_CHANNELS", 1))
    knob("AR_SLICES", kn.get("AR_SLICES", 0))
    knob("SCAN_PP", kn.get("SCAN_PP", 1))
    knob("LINEAR", kn.get("LINEAR", 0))


def up(g):
    """Device copy of a guarded image; the payload lands g.lo bytes past a 256-B boundary."""
    t = torch.empty(g.image.size, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % F.ALIGN == 0, hex(t.data_ptr())
    t.copy_(torch.from_numpy(g.image))
    return t


def P(t, g):
    return ctypes.c_void_p(t.data_ptr() + g.lo)


def call(c, sg, st, rg, rt):
    coll = c["coll"]
    h = M.DTYPES[c["dtype"]][0]
    op = M.OPS[c["op"]] if c["op"] else 0
    send = P(st, sg) if sg is not None else IN_PLACE
    recv = P(rt, rg)
    count = c["count"]
    if coll == "allreduce":
        return L.mpigx_allreduce(send, recv, count, h, op, cv)
    if coll == "scan":
        return L.mpigx_scan(send, recv, count, h, op, cv)
    if coll == "exscan":
        return L.mpigx_exscan(send, recv, count, h, op, cv)
    if coll == "reduce":
        return L.mpigx_reduce(send, recv, count, h, op, c["root"], cv)
    if coll == "bcast":
        return L.mpigx_bcast(recv, count, h, c["root"], cv)
    if coll in ("allgather", "alltoall"):
        f = L.mpigx_allgather if coll == "allgather" else L.mpigx_alltoall
        if sg is None:
            return f(IN_PLACE, 0, 0, recv, count, h, cv)
        return f(send, count, h, recv, count, h, cv)
    if coll == "reduce_scatter_block":
        return L.mpigx_reduce_scatter_block(send, recv, count, h, op, cv)
    return L.mpigx_reduce_scatter(send, recv, (ctypes.c_int * n)(*c["counts"]), h, op, cv)


def run(c):
    apply_knobs(c["knobs"])
    ins = F.inputs(c, n)
    outs = F.expected(c, n, ins)
    sg, rg = F.buffers(c, n, r, ins, outs)
    st = up(sg) if sg is not None else None
    rt = up(rg)
    if STREAM:
        torch.cuda.synchronize()
    rc = call(c, sg, st, rg, rt)
    if STREAM and rc == 0:
        rc = L.mpigx_comm_synchronize(cv)
    tag = {k: c[k] for k in ("id", "coll", "path", "dtype", "op", "count", "root", "inplace")}
    RAN[0] += 1
    if rc != 0:
        FAIL.append(dict(tag, kind="rc", rc=int(rc)))
        return
    for what, g, t in (("recv", rg, rt), ("send", sg, st)):
        if g is None:
            continue
        RAN[0] += 1
        for f in F.verify(g, t.cpu().numpy()):
            FAIL.append(dict(tag, buf=what, off=g.lo - F.PRE, **f))


knob("AR_TUNE", 0)
knob("BYTES_PER_BLOCK", 16)
if STREAM:
    assert L.mpigx_comm_set_blocking(cv, 0) == 0
table = {"main": F.cases, "small": F.small_arena_cases, "complex": F.complex_cases}[TABLE](n)
if TABLE == "small":
    assert MPI.get_knob(comm, "STAGING_BYTES") == F.SMALL_STAGE, MPI.get_knob(comm, "STAGING_BYTES")
for c in table:
    run(c)
if STREAM:
    assert L.mpigx_comm_set_blocking(cv, 1) == 0
apply_knobs({})
hits, exch = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
L.mpigx_comm_zc_stats(cv, ctypes.byref(hits), ctypes.byref(exch))
MPI.Barrier(comm)
MPI.Finalize()
print(json.dumps({"rank": r, "n": n, "table": TABLE, "cases": len(table), "checks": RAN[0], "nfail": len(FAIL),
                  "failures": FAIL[:8], "zc_exchanges": exch.value, "zc_hits": hits.value}), flush=True)
sys.exit(1 if FAIL else 0)
