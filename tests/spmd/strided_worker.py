"""Derived datatypes in Gatherv / Scatterv / Allgatherv / Alltoallv and in
one-sided Get / Put: this rank's share of tests/spmd/strided_cases.py `ops(n)`.

Run as N ranks.  MPIGX_TEST_ARRAYTYPE=ROCArray puts every buffer on the rank's
GPU (libmpigx: copy.hip seg_pack_kernel / typed_xfer_kernel); otherwise the
buffers are numpy arrays on host libmpi (MPICH 3.3.2 under mpiexec).  Each
rank writes one JSON record list; the host run's records are the fixture
(tests/golden/make_strided_golden.sh -> tests/golden/strided_golden.json) that
the device run must reproduce byte for byte (tests/test_strided_gpu.py).
Records are hex dumps of whole buffers, which start as 0xEE, so the bytes a
type map does not cover are checked too.

Device run only (DEV_CHECKS): the error classes of a Put / Get whose sides
disagree in size, of a target type past the engine's run capacity, and of a
typed access past the window."""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "mpi.jl_amd"))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import mpigx as MPI  # noqa: E402
import strided_cases as SC  # noqa: E402

DEVICE = os.environ.get("MPIGX_TEST_ARRAYTYPE", "") == "ROCArray"
if DEVICE:
    import torch

REC = []
DEV_CHECKS = []
comm = MPI.Init()
rank, n = MPI.Comm_rank(comm), MPI.Comm_size(comm)
TYPES = {}


def dev(a):
    a = np.ascontiguousarray(a)
    if DEVICE:
        return torch.from_numpy(a.copy()).to(f"cuda:{comm.device}")
    return a.copy()


def hexof(x):
    if x is None:
        return None
    if DEVICE:
        torch.cuda.synchronize()
        x = x.cpu().numpy()
    return SC.hexof(x)


def dt(spec):
    key = repr(spec)
    if key not in TYPES:
        TYPES[key] = SC.build(MPI, spec)
    return TYPES[key]


def operand(s):
    """(array, MPI.Buffer factory) of one side, or (None, None)."""
    if s is None:
        return None, lambda count: None
    arr = dev(s["buf"])
    return arr, lambda count: MPI.Buffer(arr[s["off"]:], count, dt(s["spec"]))


def collective(op):
    me, counts, root = op["ranks"][rank], op["counts"], op["root"]
    _, send = operand(me["send"])
    rarr, recv = operand(me["recv"])
    kind = op["kind"]
    if kind == "gatherv":
        MPI.Gatherv_(send(counts[rank]), recv(sum(counts)), counts, root, comm)
    elif kind == "scatterv":
        MPI.Scatterv_(send(sum(counts)), recv(counts[rank]), counts, root, comm)
    elif kind == "allgatherv":
        if me["send"] is None:
            MPI.Allgatherv_(recv(sum(counts)), counts, comm)
        else:
            MPI.Allgatherv_(send(counts[rank]), recv(sum(counts)), counts, comm)
    else:
        rc = [counts[p][rank] for p in range(n)]
        MPI.Alltoallv_(send(sum(counts[rank])), recv(sum(rc)), counts[rank], rc, comm)
    REC.append({"case": op["name"], "recv": hexof(rarr)})


def err_class(f):
    try:
        f()
    except MPI.MPIError as e:
        return MPI.Error_class(e.code)
    return 0


def rma(op):
    win_arr, dyn_arr = dev(op["win"][rank]), dev(op["dyn"][rank])
    win = MPI.Win_create(win_arr, comm)
    dwin = MPI.Win_create_dynamic(comm)
    MPI.Win_attach(dwin, dyn_arr)
    mine = dev(np.array([MPI.Get_address(dyn_arr)], dtype=np.int64))
    every = dev(np.zeros(n, dtype=np.int64))
    MPI.Allgather_(mine, every, 1, comm)
    if DEVICE:
        torch.cuda.synchronize()
    addr = [int(a) for a in (every.cpu().numpy() if DEVICE else every)]

    def go(x, buf):
        w = dwin if x["dyn"] else win
        disp = x["disp"] + (addr[x["target"]] if x["dyn"] and x["target"] >= 0 else 0)
        f = MPI.Put if x["what"] == "put" else MPI.Get
        f(MPI.Buffer(buf, x["ocount"], dt(x["ospec"])), x["ocount"], x["target"], disp, w,
          target=(x["tcount"], dt(x["tspec"])))

    MPI.Win_fence(0, win)
    MPI.Win_fence(0, dwin)
    keep = []
    for x in op["puts"]:
        if x["origin"] == rank:
            keep.append(dev(x["obuf"]))
            go(x, keep[-1])
    MPI.Win_fence(0, win)
    MPI.Win_fence(0, dwin)
    got = []
    for x in op["gets"]:
        if x["origin"] == rank:
            got.append(dev(x["obuf"]))
            go(x, got[-1])
    MPI.Win_fence(0, win)
    MPI.Win_fence(0, dwin)
    REC.append({"case": op["name"], "win": hexof(win_arr), "dyn": hexof(dyn_arr), "gets": [hexof(g) for g in got]})
    if DEVICE:
        i4 = np.dtype("i4")
        t = (rank + 1) % n
        src = dev(SC.data(4096, 7))
        vec = ("vector", 3, 2, 4, i4)
        before = hexof(win_arr)
        # the sides describe different numbers of bytes
        for f in (MPI.Put, MPI.Get):
            DEV_CHECKS.append({"check": f"{f.__name__}_size_mismatch", "want": MPI.consts.MPI_ERR_TYPE, "got": err_class(
                lambda: f(MPI.Buffer(src, 1, dt(vec)), 1, t, 0, win, target=(5, dt(i4))))})
        # a target type of 65 runs (a 3-D subarray of 64 runs is accepted below): refused at the call
        big = ("subarray", (65, 3, 4), (65, 2, 2), (0, 1, 1), np.dtype("u1"))
        DEV_CHECKS.append({"check": "Put_run_capacity", "want": MPI.consts.MPI_ERR_TYPE, "got": err_class(
            lambda: MPI.Put(MPI.Buffer(src, 260, dt(np.dtype("u1"))), 260, t, 0, win, target=(1, dt(big))))})
        # a typed access whose true bounds pass the end of the window
        for f in (MPI.Put, MPI.Get):
            DEV_CHECKS.append({"check": f"{f.__name__}_past_window", "want": MPI.consts.MPI_ERR_RMA_RANGE, "got": err_class(
                lambda: f(MPI.Buffer(src, 1, dt(vec)), 1, t, SC.WIN_BYTES - 36, win, target=(1, dt(vec))))})
        MPI.Win_fence(0, win)
        DEV_CHECKS.append({"check": "refused_calls_wrote_nothing", "want": before, "got": hexof(win_arr)})
        # 64 runs: the stated capacity
        cube = ("subarray", (64, 3, 4), (64, 2, 2), (0, 1, 1), np.dtype("u1"))
        MPI.Put(MPI.Buffer(src, 256, dt(np.dtype("u1"))), 256, t, 0, win, target=(1, dt(cube)))
        MPI.Win_fence(0, win)
        want = SC.blank(SC.WIN_BYTES)
        want[:] = np.frombuffer(bytes.fromhex(before), np.uint8)
        SC.unpack(want, SC.data(4096, 7)[:256], cube, 1)
        DEV_CHECKS.append({"check": "Put_64_runs", "want": SC.hexof(want), "got": hexof(win_arr)})
    MPI.Win_detach(dwin, dyn_arr)
    MPI.win_free(dwin)
    MPI.win_free(win)


failed = None
try:
    for op in SC.ops(n):
        (rma if op["kind"] == "rma" else collective)(op)
        MPI.Barrier(comm)
except Exception:  # noqa: BLE001
    failed = traceback.format_exc()
_line = json.dumps({"rank": rank, "n": n, "device": DEVICE, "records": REC, "failed": failed,
                    "dev_checks": DEV_CHECKS})
with open(f"{os.environ['DT_OUT']}.{rank}", "w") as f:
    f.write(_line + "\n")
MPI.Finalize()
sys.exit(1 if failed else 0)
