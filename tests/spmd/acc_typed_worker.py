"""SPMD worker: Accumulate / Get_accumulate through non-contiguous derived
datatypes — the table of tests/spmd/acc_typed_cases.py through the mirror
(MPI.Buffer operands and `target=`).

Run as N ranks.  MPIGX_TEST_ARRAYTYPE=ROCArray puts every window and operand
on the rank's GPU (libmpigx: acc_typed_kernel); otherwise they are numpy
arrays on host libmpi (MPICH 3.3.2 under mpiexec, MPIGX_HOST_ONLY=1), which
skips the cases MPICH cannot express (bf16) and the refusals.  The host run's
records are the fixture (tests/golden/make_acc_typed_golden.sh ->
tests/golden/acc_typed_golden.json) that the device run must reproduce.

One window per element type is created once and refilled before every case;
each case is one fence epoch.  A record holds the return class and the WHOLE
window, result allocation and origin allocation after the case
(acc_typed_cases.enc).  The worker also compares each of them with the model
and reports the first differing element.  Prints one JSON line (or writes
$ACC_TYPED_OUT.<rank>)."""
import json
import os
import sys
import time
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "mpi.jl_amd"), os.path.join(ROOT, "tests"), HERE):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import mpigx as MPI  # noqa: E402
import acc_typed_cases as C  # noqa: E402

DEVICE = os.environ.get("MPIGX_TEST_ARRAYTYPE", "") == "ROCArray"
if DEVICE:
    import torch

T0 = time.time()
comm = MPI.Init()
rank, n = MPI.Comm_rank(comm), MPI.Comm_size(comm)
tgt = (rank + 1) % n

REC, FAILS, REFUSED = [], [], []
_TYPES = {}


def A(a):
    """The numpy array as an operand of this run: a device tensor of the same
    bits (bf16 travels as uint16 bit patterns) or a host copy."""
    if not DEVICE:
        return np.array(a, copy=True)
    raw = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(f"cuda:{comm.device}")
    return raw.view(torch.bfloat16 if a.dtype == np.uint16 else getattr(torch, a.dtype.name))


def H(x):
    """Host copy of an operand, bits as the numpy type of the table."""
    if isinstance(x, np.ndarray):
        return x.copy()
    torch.cuda.synchronize()
    return x.view(torch.uint8).cpu().numpy()


def upload(buf, a):
    if isinstance(buf, np.ndarray):
        buf[:] = a
    else:
        buf.view(torch.uint8).copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)))


def dtype_of(desc, tname):
    key = (json.dumps(desc, sort_keys=True), tname)
    if key not in _TYPES:
        _TYPES[key] = C.build(MPI, desc, tname)
    return _TYPES[key]


def side(buf, s, tname):
    return MPI.Buffer(buf, s[1], dtype_of(s[0], tname))


def err_class(fn):
    try:
        fn()
    except MPI.MPIError as e:
        return MPI.Error_class(e.code)
    return 0


def differ(c, part, got, want):
    got, want = got.view(np.uint8).reshape(-1), want.view(np.uint8).reshape(-1)
    if got.size == want.size and np.array_equal(got, want):
        return
    i = int(np.flatnonzero(got != want)[0]) if got.size == want.size else -1
    FAILS.append({"case": c["id"], "part": part, "byte": i, "element": i // C.esize(c.get("type", "int8"))})


def issue(c, win, disp, target_rank, j=0, shift=0):
    """One Accumulate / Get_accumulate of the case; (class, origin, result)."""
    tn = c["type"]
    ob = A(C.origin_buffer(c, rank, j))
    rb = A(C.result_buffer(c)) if c["r"] else None
    op = getattr(MPI, c["op"].split("+")[j])
    T = side(None, c["t"], tn)
    if c["kind"] == "acc":
        rc = err_class(lambda: MPI.Accumulate(side(ob, c["o"], tn), None, target_rank, disp + shift, op, win, target=T))
    else:
        rc = err_class(lambda: MPI.Get_accumulate(side(ob, c["o"], tn), side(rb, c["r"], tn), None, target_rank,
                                                  disp + shift, op, win, target=T))
    return rc, ob, rb


def run_case(c, wbuf, win, length, disp):
    upload(wbuf, C.window_init(c, rank, n, length))
    MPI.Win_fence(0, win)
    if c["shape"] == "order":
        posts = [issue(c, win, disp, tgt, j, j * C.ORDER_SHIFT) for j in range(2)]
    else:
        posts = [issue(c, win, disp, 0 if c["shape"] == "multi" else tgt)]
    MPI.Win_fence(0, win)
    got_win = H(wbuf)
    want_win, want_res = C.model(c, rank, n, length)
    differ(c, "window", got_win, want_win)
    rec = {"case": c["id"], "rc": [p[0] for p in posts], "window": C.enc(got_win), "result": None, "origin": []}
    for j, (rc, ob, rb) in enumerate(posts):
        if rc:
            FAILS.append({"case": c["id"], "part": f"rc of post {j}", "byte": rc, "element": rc})
        got_o = H(ob)
        differ(c, "origin", got_o, C.origin_buffer(c, rank, j))
        rec["origin"].append(C.enc(got_o))
        if rb is not None:
            got_r = H(rb)
            differ(c, "result", got_r, want_res)
            rec["result"] = C.enc(got_r)
    REC.append(rec)


def run_dynamic(c):
    es = C.esize(c["type"])
    wbuf = A(C.sentinel(c["type"], c["wlen"]))
    win = MPI.Win_create_dynamic(comm)
    MPI.Win_attach(win, wbuf)
    addrs = H(MPI.Allgather(A(np.array([MPI.Get_address(wbuf)], np.int64)), comm)).view(np.int64)
    run_case(c, wbuf, win, c["wlen"], int(addrs[tgt]) + c["disp"] * es)  # absolute address of the displacement
    MPI.Barrier(comm)
    MPI.Win_detach(win, wbuf)
    MPI.free(win)


def run_refusals(windows):
    """Engine only: the call returns the listed class and the window (as this
    rank's, and so as its origin's target) keeps every sentinel byte."""
    for r in C.REFUSALS:
        wbuf, win, length = windows[r["ttype"]]
        upload(wbuf, C.sentinel(r["ttype"], length))
        MPI.Win_fence(0, win)
        ob = A(np.zeros(r["o"][1], C.npdt(r["otype"])))
        O = MPI.Buffer(ob, r["o"][1], getattr(MPI, C.MPI_TYPE[r["otype"]]))
        if r.get("mixed"):
            T = MPI.Buffer(None, 1, MPI.Types.commit_(MPI.Types.create_struct([2, 2], [0, 12], [MPI.INT32_T, MPI.FLOAT])))
        else:
            T = side(None, r["t"], r["ttype"])
        disp = length - 5 if r.get("past") else C.GUARD
        rc = err_class(lambda: MPI.Accumulate(O, None, tgt, disp, MPI.REPLACE, win, target=T))
        MPI.Win_fence(0, win)
        got = H(wbuf)
        untouched = bool((got.view(np.uint8) == C.SENTINEL).all())
        REFUSED.append({"case": r["id"], "rc": rc, "want": r["want"], "untouched": untouched})
        if rc != r["want"] or not untouched:
            FAILS.append({"case": r["id"], "part": "refusal", "byte": rc, "element": int(untouched)})


def main():
    windows = {}
    for tn in dict.fromkeys(c["type"] for c in C.CASES):
        if not DEVICE and tn == "bfloat16":
            continue
        length = C.window_elems(tn)
        wbuf = A(C.sentinel(tn, length))
        windows[tn] = (wbuf, MPI.Win_create(wbuf, comm), length)
    for c in C.CASES:
        if not DEVICE and not c["mpich"]:
            continue
        if c["dyn"]:
            run_dynamic(c)
        else:
            wbuf, win, length = windows[c["type"]]
            run_case(c, wbuf, win, length, c["disp"])
    if DEVICE:
        run_refusals(windows)
    MPI.Barrier(comm)
    for _, win, _ in windows.values():
        MPI.free(win)


failed = None
try:
    main()
except Exception:  # noqa: BLE001
    failed = traceback.format_exc()
_line = json.dumps({"rank": rank, "n": n, "device": DEVICE, "records": REC, "refused": REFUSED, "nfail": len(FAILS),
                    "first_failures": FAILS[:8], "failed": failed, "seconds": round(time.time() - T0, 2)})
if os.environ.get("ACC_TYPED_OUT"):  # one file per rank (long lines from several ranks interleave on a pipe)
    with open(f"{os.environ['ACC_TYPED_OUT']}.{rank}", "w") as f:
        f.write(_line + "\n")
else:
    print(_line, flush=True)
if failed is None:
    MPI.Finalize()
sys.exit(1 if failed else 0)
