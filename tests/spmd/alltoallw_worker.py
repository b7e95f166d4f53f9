"""Alltoallw: this rank's share of tests/spmd/alltoallw_cases.py `ops(n)`.

Run as N ranks.  MPIGX_TEST_ARRAYTYPE=ROCArray puts every buffer on the rank's
GPU (libmpigx: mpigx_alltoallw, copy.hip segw_pack_kernel); otherwise the
buffers are numpy arrays on host libmpi (MPICH 3.3.2's MPI_Alltoallw under
mpiexec).  Each rank writes one JSON record list; the host run's records are
the fixture (tests/golden/make_alltoallw_golden.sh ->
tests/golden/alltoallw_golden.json) that the device run must reproduce byte
for byte (tests/test_alltoallw_gpu.py).  A record is the hex dump of the WHOLE
receive allocation, which starts as a position-dependent sentinel, so the
bytes no type map covers are checked too; the send allocation must come back
unchanged.

Device run only, by ATW_MODE:
  full    the table, the refusals (every rank makes the same refused call;
          error class, both allocations untouched, the next call still exact),
          then on rank 0 the kernel-geometry cases through the diagnostic
          entry point mpigx_pack_segments_w, against the model
  rounds  one typed call whose blocks are several staging rounds long (the
          launcher passes a small MPIGX_STAGING_BYTES)
  stream  one stream-ordered call (mpigx_comm_set_blocking 0), checked after
          mpigx_comm_synchronize"""
import ctypes
import json
import os
import sys
import time
import traceback

T0 = time.perf_counter()

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "mpi.jl_amd"))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import mpigx as MPI  # noqa: E402
import alltoallw_cases as AC  # noqa: E402
import strided_cases as SC  # noqa: E402

DEVICE = os.environ.get("MPIGX_TEST_ARRAYTYPE", "") == "ROCArray"
MODE = os.environ.get("ATW_MODE", "full")
if DEVICE:
    import torch

REC = []
DEV_CHECKS = []
SECONDS = {"import": round(time.perf_counter() - T0, 3)}  # since process start, for the suite's time budget
comm = MPI.Init()
SECONDS["init"] = round(time.perf_counter() - T0, 3)
rank, n = MPI.Comm_rank(comm), MPI.Comm_size(comm)
TYPES = {}
K = MPI.consts


def dev(a):
    a = np.ascontiguousarray(a)
    if DEVICE:
        return torch.from_numpy(a.copy()).to(f"cuda:{comm.device}")
    return a.copy()


def host(x):
    return x.cpu().numpy() if DEVICE else x  # (the copy waits for the stream)


def dt(spec):
    key = repr(spec)
    if key not in TYPES:
        TYPES[key] = SC.build(MPI, spec)
    return TYPES[key]


def args_of(s):
    """(allocation, pointer view, counts, displs, types) of one side."""
    if s is None:
        return None, MPI.IN_PLACE, None, None, None
    arr = dev(s["buf"])
    return (arr, arr[s["off"]:], [c for c, _, _ in s["blocks"]], [d for _, d, _ in s["blocks"]],
            [dt(t) for _, _, t in s["blocks"]])


def run(op):
    me = op["ranks"][rank]
    sarr, sptr, sc, sd, st = args_of(me["send"])
    rarr, rptr, rc, rd, rt = args_of(me["recv"])
    MPI.Alltoallw_(sptr, sc, sd, st, rptr, rc, rd, rt, comm)
    return sarr, rarr


def collective(op):
    me = op["ranks"][rank]
    sarr, rarr = run(op)
    REC.append({"case": op["name"], "recv": SC.hexof(host(rarr)),
                "send_unchanged": sarr is None or bool(np.array_equal(host(sarr), me["send"]["buf"]))})


def ints(xs):
    return (ctypes.c_int * len(xs))(*[int(x) for x in xs])


def refusals(op):
    """Every refusal of mpigx_alltoallw, made by every rank in the same call."""
    L = MPI.lib()
    me = op["ranks"][rank]
    sarr, sptr, sc, sd, st = args_of(me["send"])
    rarr, rptr, rc, rd, rt = args_of(me["recv"])
    sp, rp = ctypes.c_void_p(sptr.data_ptr()), ctypes.c_void_p(rptr.data_ptr())
    good = [ints(sc), ints(sd), ints([t.val for t in st]), ints(rc), ints(rd), ints([t.val for t in rt])]
    assert any(sc) and any(rc)
    MPI.api._stream(comm)

    def refused(name, want, send=sp, recv=rp, c=comm.val, **swap):
        a = list(good)
        for k, v in swap.items():
            a[int(k[1:])] = v
        got = L.mpigx_alltoallw(send, a[0], a[1], a[2], recv, a[3], a[4], a[5], c)
        DEV_CHECKS.append({"check": name, "want": want, "got": got})

    for k, nm in enumerate(("sendcounts", "sdispls", "sendtypes", "recvcounts", "rdispls", "recvtypes")):
        refused(f"null_{nm}", K.MPI_ERR_ARG, **{f"a{k}": None})
    neg = list(sc)
    neg[(rank + 1) % n] = -1
    refused("negative_sendcount", K.MPI_ERR_COUNT, a0=ints(neg))
    neg = list(rc)
    neg[rank] = -3
    refused("negative_recvcount", K.MPI_ERR_COUNT, a3=ints(neg))
    # a bad type in a slot whose count is 0 is refused all the same
    zero = list(rc)
    zero[0] = 0
    T = MPI.Types
    uncommitted = T.create_vector(2, 1, 3, MPI.Datatype(np.dtype("i4")))
    freed = T.commit_(T.create_vector(2, 1, 5, MPI.Datatype(np.dtype("i4"))))
    stale = freed.val
    h = ctypes.c_int(stale)
    assert L.mpigx_type_free(ctypes.byref(h)) == 0
    for nm, bad in (("unknown", 12345), ("uncommitted", uncommitted.val), ("freed", stale)):
        types = [t.val for t in rt]
        types[0] = bad
        refused(f"{nm}_type_in_an_empty_slot", K.MPI_ERR_TYPE, a3=ints(zero), a5=ints(types))
    types = [t.val for t in st]
    types[n - 1] = 12345
    refused("unknown_sendtype", K.MPI_ERR_TYPE, a2=ints(types))
    refused("null_recvbuf", K.MPI_ERR_BUFFER, recv=None)
    refused("null_sendbuf", K.MPI_ERR_BUFFER, send=None)
    refused("null_comm", K.MPI_ERR_COMM, c=None)
    DEV_CHECKS.append({"check": "refused_calls_wrote_nothing", "want": True,
                       "got": bool(np.array_equal(host(sarr), me["send"]["buf"]) and
                                   np.array_equal(host(rarr), me["recv"]["buf"]))})


def exact(op, name, want):
    """Runs `op` and compares with the model's record."""
    sarr, rarr = run(op)
    if MODE == "stream":
        MPI.api._check(MPI.lib().mpigx_comm_synchronize(comm.val))
    DEV_CHECKS.append({"check": name, "want": want["recv"], "got": SC.hexof(host(rarr))})


def geometry():
    L = MPI.lib()
    LL = ctypes.c_longlong
    for g in AC.geometry():
        tb, off, pb = AC.geometry_buffers(g)
        typed0, packed0 = SC.data(tb, 5), AC.sentinel(pb, 9)
        ns = len(g["segs"])
        types = ints([dt(t).val for t, _, _, _ in g["segs"]])
        counts = (LL * ns)(*[c for _, c, _, _ in g["segs"]])
        displs = (LL * ns)(*[d for _, _, d, _ in g["segs"]])
        offs = (LL * ns)(*[o for _, _, _, o in g["segs"]])
        for unpack in (0, 1):
            typed, packed = dev(typed0), dev(packed0)
            w = ints([-1] * ns)
            rc = L.mpigx_pack_segments_w(ctypes.c_void_p(typed.data_ptr() + off), ns, types, counts, displs, offs,
                                         ctypes.c_void_p(packed.data_ptr()), unpack, w, None)
            assert rc == 0, (g["name"], unpack, rc)
            want = AC.geometry_expected(g, typed0, packed0, unpack)
            t, p = host(typed), host(packed)
            ok = (np.array_equal(t, want) and np.array_equal(p, packed0)) if unpack else \
                (np.array_equal(p, want) and np.array_equal(t, typed0))
            model_w = [AC.unit_width(s, c, typed.data_ptr() + off + d, packed.data_ptr() + o)
                       for s, c, d, o in g["segs"]]
            DEV_CHECKS.append({"check": f"geometry_{g['name']}_{'unpack' if unpack else 'pack'}",
                               "want": [True, g["want_w"], g["want_w"]], "got": [bool(ok), list(w), model_w]})


failed = None
try:
    table = AC.ops(n)
    if MODE == "full" or not DEVICE:
        for op in table:
            collective(op)
        SECONDS["table"] = round(time.perf_counter() - T0, 3)
    if DEVICE and MODE == "full":
        refusals(table[3])
        exact(table[0], "exact_after_refusals", AC.play(table[0])[rank])
        SECONDS["refusals"] = round(time.perf_counter() - T0, 3)
        if rank == 0:
            geometry()
        SECONDS["geometry"] = round(time.perf_counter() - T0, 3)
        MPI.Barrier(comm)  # nobody finalizes while rank 0 is still at work
    elif DEVICE and MODE == "rounds":
        op = AC.rounds(n)
        exact(op, "rounds", AC.play(op)[rank])
    elif DEVICE and MODE == "stream":
        MPI.api._check(MPI.lib().mpigx_comm_set_blocking(comm.val, 0))
        exact(table[2], "stream_ordered", AC.expected(n)[rank][2])
        MPI.api._check(MPI.lib().mpigx_comm_set_blocking(comm.val, 1))
        MPI.Barrier(comm)
except Exception:  # noqa: BLE001
    failed = traceback.format_exc()
_line = json.dumps({"rank": rank, "n": n, "device": DEVICE, "records": REC, "failed": failed,
                    "dev_checks": DEV_CHECKS, "seconds": SECONDS})
with open(f"{os.environ['DT_OUT']}.{rank}", "w") as f:
    f.write(_line + "\n")
MPI.Finalize()
sys.exit(1 if failed else 0)
