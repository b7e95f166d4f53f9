"""Refusals of Gather, Gatherv, Scatter, Scatterv, Allgatherv and Alltoallv on
device buffers, through the raw C ABI (tests/test_vcoll_refusals_gpu.py).

Run as N ranks.  EVERY rank makes the same refused call, so that nobody goes
on into the host exchange and waits: an argument that only the root reads (a
null recvcounts at a Gatherv root, a negative recvcount of Gather) is not in
the table, and the IN_PLACE-at-a-non-root rows give every rank the root
(rank + 1) % n.

Each row is made twice:
  i4   int32 on both sides, 5 elements per block
  vec  the committed vector(2, 1, 3, int32) (8 bytes in a 16-byte extent), 5
       instances per block, on the side the row names (`vec=`), and int32, 10
       elements per block, on the other side, which is the layout of a valid
       call; a row about a bad type handle puts the vector on the OTHER side
so the table covers the in-place and the packed side alike.  Gather and
Scatter pack a derived type with the whole-buffer pack_kernel, a route of
their own that packs a null buffer without looking at it; their null-buffer
rows are i4 only.

VCR_SKIP (comma-separated row names) leaves rows out: a library from before
null buffers were refused on every route would launch vx_kernel on the null
pointer in the rows of test_vcoll_refusals_gpu.TIGHTENED.

After the table: the guard-padded send and receive allocations every call
pointed into are byte-identical to their initial contents, and one valid
Alltoallv is exact."""
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
import torch  # noqa: E402

import mpigx as MPI  # noqa: E402
import strided_cases as SC  # noqa: E402

SKIP = set(filter(None, os.environ.get("VCR_SKIP", "").split(",")))
CHECKS = []
SECONDS = {"import": round(time.perf_counter() - T0, 3)}
comm = MPI.Init()
SECONDS["init"] = round(time.perf_counter() - T0, 3)
rank, n = MPI.Comm_rank(comm), MPI.Comm_size(comm)
K = MPI.consts
L = MPI.lib()
GUARD, ROOM = 64, 512  # a side of n = 3 blocks of 5 vector instances spans 240 bytes


def ints(xs):
    return (ctypes.c_int * len(xs))(*[int(x) for x in xs])


ORDER = {
    "gather": ("send", "scount", "stype", "recv", "rcount", "rtype", "root", "comm"),
    "gatherv": ("send", "scount", "stype", "recv", "rcounts", "rdispls", "rtype", "root", "comm"),
    "scatter": ("send", "scount", "stype", "recv", "rcount", "rtype", "root", "comm"),
    "scatterv": ("send", "scounts", "sdispls", "stype", "recv", "rcount", "rtype", "root", "comm"),
    "allgatherv": ("send", "scount", "stype", "recv", "rcounts", "rdispls", "rtype", "comm"),
    "alltoallv": ("send", "scounts", "sdispls", "stype", "recv", "rcounts", "rdispls", "rtype", "comm"),
}
ROOTED = ("gather", "gatherv", "scatter", "scatterv")
ARRAYS = ("scounts", "sdispls", "rcounts", "rdispls")


def main():
    I4 = MPI.Datatype(np.dtype("i4")).val
    VEC = SC.build(MPI, ("vector", 2, 1, 3, np.dtype("i4"))).val
    T = MPI.Types
    uncommitted = T.create_vector(2, 1, 3, MPI.Datatype(np.dtype("i4")))
    freed = T.commit_(T.create_vector(2, 1, 5, MPI.Datatype(np.dtype("i4"))))
    stale = freed.val
    h = ctypes.c_int(stale)
    assert L.mpigx_type_free(ctypes.byref(h)) == 0
    bad_types = (("unknown", 12345), ("uncommitted", uncommitted.val), ("freed", stale))

    send0, recv0 = SC.data(GUARD + ROOM + GUARD, 1 + rank), SC.data(GUARD + ROOM + GUARD, 11 + rank)
    dev = f"cuda:{comm.device}"
    sarr, rarr = torch.from_numpy(send0.copy()).to(dev), torch.from_numpy(recv0.copy()).to(dev)
    sp, rp = ctypes.c_void_p(sarr.data_ptr() + GUARD), ctypes.c_void_p(rarr.data_ptr() + GUARD)
    in_place = ctypes.c_void_p(-1 & ((1 << 64) - 1))
    MPI.api._stream(comm)

    def base(vec):
        """Python-side arguments of a valid call; vec: None, "send" or "recv"."""
        cnt = {"send": 5, "recv": 5}
        typ = {"send": I4, "recv": I4}
        if vec:
            typ[vec] = VEC
            cnt["recv" if vec == "send" else "send"] = 10
        return {"send": sp, "recv": rp, "stype": typ["send"], "rtype": typ["recv"], "root": 0, "comm": comm.val,
                "scount": cnt["send"], "rcount": cnt["recv"],
                "scounts": [cnt["send"]] * n, "sdispls": [q * cnt["send"] for q in range(n)],
                "rcounts": [cnt["recv"]] * n, "rdispls": [q * cnt["recv"] for q in range(n)]}

    def refused(coll, name, want, vec, variants=("i4", "vec"), **swap):
        """swap: argument name -> value, or a function of the valid arguments."""
        for variant in variants:
            row = f"{coll}_{name}_{variant}"
            if row in SKIP:
                continue
            a = base(vec if variant == "vec" else None)
            for k, v in swap.items():
                a[k] = v(a) if callable(v) else v
            keep = [ints(a[k]) if k in ARRAYS and a[k] is not None else a[k] for k in ORDER[coll]]
            got = getattr(L, f"mpigx_{coll}")(*keep)
            CHECKS.append({"check": row, "want": want, "got": got})

    def with_at(key, at, value):
        return lambda a: [value if q == at else x for q, x in enumerate(a[key])]

    for coll in ORDER:
        side = "send" if coll in ("gather", "gatherv") else "recv"  # a side every rank reads
        other = "recv" if side == "send" else "send"
        refused(coll, "null_comm", K.MPI_ERR_COMM, side, comm=None)
        if coll in ROOTED:
            refused(coll, "root_n", K.MPI_ERR_ROOT, side, root=n)
            refused(coll, "root_minus_1", K.MPI_ERR_ROOT, side, root=-1)
            refused(coll, "in_place_on_a_non_root", K.MPI_ERR_BUFFER, side, root=(rank + 1) % n,
                    **{side: in_place})
        # the side of a rooted call that every rank reads is one block: (buffer, count, type)
        one = {"send": ("send", "scount", "stype"), "recv": ("recv", "rcount", "rtype")}[side]
        if coll in ROOTED:
            refused(coll, f"negative_{one[1]}", K.MPI_ERR_COUNT, side, **{one[1]: -1})
            for nm, bad in bad_types:
                refused(coll, f"{nm}_{one[2]}", K.MPI_ERR_TYPE, other, **{one[2]: bad})
            refused(coll, f"null_{one[0]}buf", K.MPI_ERR_BUFFER, side,
                    variants=("i4",) if coll in ("gather", "scatter") else ("i4", "vec"), **{one[0]: None})
    # Allgatherv: recvcounts / displs are read by every rank
    refused("allgatherv", "null_recvcounts", K.MPI_ERR_ARG, "recv", rcounts=None)
    refused("allgatherv", "null_displs", K.MPI_ERR_ARG, "recv", rdispls=None)
    refused("allgatherv", "negative_recvcount", K.MPI_ERR_COUNT, "recv", rcounts=with_at("rcounts", rank, -3))
    refused("allgatherv", "negative_sendcount", K.MPI_ERR_COUNT, "send", scount=-1)
    for nm, bad in bad_types:
        refused("allgatherv", f"{nm}_recvtype", K.MPI_ERR_TYPE, "send", rtype=bad)
        refused("allgatherv", f"{nm}_sendtype", K.MPI_ERR_TYPE, "recv", stype=bad)
    refused("allgatherv", "null_recvbuf", K.MPI_ERR_BUFFER, "recv", recv=None)
    refused("allgatherv", "null_sendbuf", K.MPI_ERR_BUFFER, "send", send=None)
    # my own block empty, the peers' not: nothing of mine lands in the null buffer, the peers' blocks would
    refused("allgatherv", "null_recvbuf_peers_only", K.MPI_ERR_BUFFER, "recv", recv=None, scount=0,
            rcounts=with_at("rcounts", rank, 0))
    # Alltoallv
    for k, nm in (("scounts", "sendcounts"), ("sdispls", "sdispls"), ("rcounts", "recvcounts"), ("rdispls", "rdispls")):
        refused("alltoallv", f"null_{nm}", K.MPI_ERR_ARG, "send" if k[0] == "s" else "recv", **{k: None})
    refused("alltoallv", "negative_sendcount", K.MPI_ERR_COUNT, "send", scounts=with_at("scounts", (rank + 1) % n, -1))
    refused("alltoallv", "negative_recvcount", K.MPI_ERR_COUNT, "recv", rcounts=with_at("rcounts", rank, -3))
    for nm, bad in bad_types:
        refused("alltoallv", f"{nm}_recvtype", K.MPI_ERR_TYPE, "send", rtype=bad)
        refused("alltoallv", f"{nm}_sendtype", K.MPI_ERR_TYPE, "recv", stype=bad)
    refused("alltoallv", "null_recvbuf", K.MPI_ERR_BUFFER, "recv", recv=None)
    refused("alltoallv", "null_sendbuf", K.MPI_ERR_BUFFER, "send", send=None)
    SECONDS["table"] = round(time.perf_counter() - T0, 3)

    untouched = np.array_equal(sarr.cpu().numpy(), send0) and np.array_equal(rarr.cpu().numpy(), recv0)
    CHECKS.append({"check": "refused_calls_wrote_nothing", "want": True, "got": bool(untouched)})

    # one valid call: rank r sends q its block q = 100 r + 10 q + j
    def block(r, q):
        return 100 * r + 10 * q + np.arange(5, dtype=np.int32)

    s = torch.from_numpy(np.concatenate([block(rank, q) for q in range(n)])).to(dev)
    d = torch.full((5 * n,), -1, dtype=torch.int32, device=dev)
    five, at = ints([5] * n), ints([5 * q for q in range(n)])
    got = L.mpigx_alltoallv(ctypes.c_void_p(s.data_ptr()), five, at, I4, ctypes.c_void_p(d.data_ptr()), five, at, I4,
                            comm.val)
    want = np.concatenate([block(q, rank) for q in range(n)])
    CHECKS.append({"check": "exact_after_refusals", "want": [0, want.tolist()], "got": [got, d.cpu().numpy().tolist()]})
    SECONDS["exact"] = round(time.perf_counter() - T0, 3)
    MPI.Barrier(comm)


failed = None
try:
    main()
except Exception:  # noqa: BLE001
    failed = traceback.format_exc()
with open(f"{os.environ['DT_OUT']}.{rank}", "w") as f:
    f.write(json.dumps({"rank": rank, "n": n, "failed": failed, "checks": CHECKS, "seconds": SECONDS}) + "\n")
MPI.Finalize()
sys.exit(1 if failed else 0)
